// flow.hip -- the Wilson gradient flow and the observables measured along it, resident on the device.  Reference caller: the driver's
// gradient-flow block after every trajectory, the reference's src/system/lqcd.jl:95-100,149-164 (Gradientflow, flow!, Energy_density,
// Topological_charge with kinds plaquette / clover / improved; defaults src/system/parameter_structs.jl:161-164).
//
// Conventions (directions 0..3 = x, y, z, t; TA(M) = (M - M^+)/2 - tr(M - M^+)/6):
//   flow      dV/dt = Z(V) V with Z = TA(G), G the staple force of lqcd_gauge_force at beta = 6 (staple.hip); one Euler step is a stout step with rho = eps.
//             Luscher's RK3 (JHEP 08 (2010) 071) with one gauge-shaped accumulator X, every stage  X <- a X + f TA(G(W)),  W <- exp(X) W:
//               (a, f) = (0, eps/4), (-17/9, 8 eps/9), (-1, 3 eps/4).
//             Single GPU: one staple sweep per stage (staple.hip flow_stage: the fused momentum + link sweep with the accumulator scaled before the add);
//             partitioned: the staple force's ghost-link / staple-face exchange, the sweep into X, then the exponential update as a second pass.
//   fields    for n closed loops through x in the (mu, nu) plane, all run the way of the plaquette +mu +nu -mu -nu:  G_mu nu(x) = TA(sum of loops) / n;
//             loop sets "plaquette" (n = 1), "clover" (the four leaves, n = 4), "rect" (the eight 1x2 and 2x1 rectangles with a corner at x, n = 8).
//   observables, in this order (LQCD_FLOW_NOBS = 6):
//     p       the plaquette of lqcd_gauge_plaquette
//     E_plaq  = 2 sum_{mu<nu} Re tr(1 - P_mu nu) per site = 36 (1 - p)
//     E_clov  = -1/2 sum_{mu,nu} tr G_mu nu G_mu nu per site (clover set)
//     Q[set]  = -1/(32 pi^2) sum_x eps_{mu nu rho sigma} tr G_mu nu G_rho sigma = -(1/4 pi^2) sum_x [tr G01 G23 - tr G02 G13 + tr G03 G12]   (eps_xyzt = +1)
//     Q_plaq  = Q[plaquette],  Q_clov = Q[clover],  Q_impr = 5/3 Q_clov - 1/12 Q_rect  with Q_rect = 2 Q[rect]
//   One launch computes every loop of a site (two planes' G held at a time), block partials go out [value][block] and one block adds them in a fixed
//   order: the results are bitwise reproducible run to run.  Partitioned lattices read the links through clover.hip's depth-1 halo-extended block
//   (corners included): the rectangles need depth 2, so Q_impr is NaN there.
#include "lqcd_internal.h"
#include "gauge_staple.h"

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace lqcd {

constexpr int FLOW_RAW = 5;                 // raw sums per measurement: sum (3 - Re tr P), -sum tr G^2 (clover), the eps contraction of each loop set
constexpr int FLOW_OBS_THREADS = 128;
constexpr double FLOW_TWO_ROW_EPS = 0.1;       // largest |eps| of a call that keeps the two-row link loads (flow_prepare)

struct ObsArgs {
    Geom g;
    const double2* U;       // single domain: the links (periodic wrap)
    const double2* ext;     // partitioned: the halo-extended block, local coordinates -1 .. L
    int E[4];
    size_t en;
    double* partial;        // [FLOW_RAW][nblk]
    int nblk;
};

template <bool EXT>
__device__ __forceinline__ void obs_link(cd (&u)[9], const ObsArgs& k, const int (&c)[4], int mu) {
    if constexpr (EXT) {
        const size_t s = (size_t)(c[0] + 1) + (size_t)k.E[0] * ((size_t)(c[1] + 1) + (size_t)k.E[1] * ((size_t)(c[2] + 1) + (size_t)k.E[2] * (size_t)(c[3] + 1)));
        const double2* b = k.ext + (size_t)mu * 9 * k.en + s;
#pragma unroll
        for (int e = 0; e < 9; e++) u[e] = ld(b + (size_t)e * k.en);
    } else {
        const int p = (c[0] + c[1] + c[2] + c[3]) & 1, Gs = glink_stride(k.g);
        const double2* b = k.U + glink_off(k.g, p, mu, coords_to_cb(k.g, c));
#pragma unroll
        for (int e = 0; e < 9; e++) u[e] = ld(b + (size_t)e * Gs);
    }
}
template <bool EXT>
__device__ __forceinline__ void obs_step(int (&c)[4], const Geom& g, int d, int dir) {
    c[d] += dir;
    if constexpr (!EXT) {
        if (c[d] == g.L[d]) c[d] = 0;
        else if (c[d] < 0) c[d] = g.L[d] - 1;
    }
}

// steps of a closed path, two bits each: 0 = +mu, 1 = +nu, 2 = -mu, 3 = -nu.  The leaf in quadrant (sm, sn) with extent a along mu and b along nu, run the
// way of the plaquette +mu +nu -mu -nu (mu first when sm sn > 0, nu first otherwise)
__device__ __forceinline__ unsigned leaf_code(int sm, int sn, int a, int b) {
    const unsigned fm = sm > 0 ? 0u : 2u, fn = sn > 0 ? 1u : 3u, bm = fm ^ 2u, bn = fn ^ 2u;
    const unsigned s1 = sm * sn > 0 ? fm : fn, s2 = sm * sn > 0 ? fn : fm, s3 = sm * sn > 0 ? bm : bn, s4 = sm * sn > 0 ? bn : bm;
    const int n1 = sm * sn > 0 ? a : b, n2 = sm * sn > 0 ? b : a;
    unsigned code = 0;
    int s = 0;
    for (int j = 0; j < n1; j++, s++) code |= s1 << (2 * s);
    for (int j = 0; j < n2; j++, s++) code |= s2 << (2 * s);
    for (int j = 0; j < n1; j++, s++) code |= s3 << (2 * s);
    for (int j = 0; j < n2; j++, s++) code |= s4 << (2 * s);
    return code;
}

// P = the product of the links along the path from x
template <bool EXT>
__device__ __forceinline__ void obs_loop(cd (&P)[9], const ObsArgs& k, const int (&x)[4], int mu, int nu, unsigned code, int n) {
    int c[4] = {x[0], x[1], x[2], x[3]};
    cd u[9], t[9];
#pragma unroll 1
    for (int s = 0; s < n; s++, code >>= 2) {
        const int d = (code & 1u) ? nu : mu;
        if (code & 2u) {
            obs_step<EXT>(c, k.g, d, -1);
            obs_link<EXT>(u, k, c, d);
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = a; b < 3; b++) {
                    const cd x1 = u[a * 3 + b], x2 = u[b * 3 + a];
                    u[a * 3 + b] = mk(x2.re, -x2.im);
                    u[b * 3 + a] = mk(x1.re, -x1.im);
                }
        } else {
            obs_link<EXT>(u, k, c, d);
            obs_step<EXT>(c, k.g, d, 1);
        }
        if (s == 0) {
#pragma unroll
            for (int e = 0; e < 9; e++) P[e] = u[e];
        } else {
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    cd acc = mk(0.0, 0.0);
#pragma unroll
                    for (int q = 0; q < 3; q++) cfma(acc, P[a * 3 + q], u[q * 3 + b]);
                    t[a * 3 + b] = acc;
                }
#pragma unroll
            for (int e = 0; e < 9; e++) P[e] = t[e];
        }
    }
}

// G = TA(sum of the loops of set `kind` in the (mu, nu) plane) / n;  retr = Re tr of the sum
template <bool EXT>
__device__ __forceinline__ void obs_field(cd (&G)[9], double& retr, const ObsArgs& k, const int (&x)[4], int mu, int nu, int kind) {
    cd S[9], P[9];
#pragma unroll
    for (int e = 0; e < 9; e++) S[e] = mk(0.0, 0.0);
    const int nl = kind == 0 ? 1 : kind == 1 ? 4 : 8;
#pragma unroll 1
    for (int l = 0; l < nl; l++) {
        const int q = kind == 2 ? l >> 1 : l;                       // quadrants (+,+) (-,+) (-,-) (+,-)
        const int sm = (q == 0 || q == 3) ? 1 : -1, sn = q < 2 ? 1 : -1;
        const int a = (kind == 2 && (l & 1)) ? 2 : 1, b = (kind == 2 && !(l & 1)) ? 2 : 1;
        obs_loop<EXT>(P, k, x, mu, nu, leaf_code(sm, sn, a, b), 2 * (a + b));
#pragma unroll
        for (int e = 0; e < 9; e++) S[e] = S[e] + P[e];
    }
    retr = S[0].re + S[4].re + S[8].re;
    ta3(G, S, 0.5 / (double)nl);
}
__device__ __forceinline__ double tr_re(const cd (&A)[9], const cd (&B)[9]) {      // Re tr A B
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) s += A[a * 3 + b].re * B[b * 3 + a].re - A[a * 3 + b].im * B[b * 3 + a].im;
    return s;
}

// one thread per site: the loop sets kind 0 (plaquette), 1 (clover), 2 (rect; single domain only) one after the other, the planes in the pairs of the eps
// contraction (01, 23) (02, 13) (03, 12) -- two G matrices live at a time
template <bool EXT>
__global__ __launch_bounds__(FLOW_OBS_THREADS) void flow_obs_kernel(ObsArgs k) {
    __shared__ double red[FLOW_RAW][FLOW_OBS_THREADS / 64];
    const int t = blockIdx.x * FLOW_OBS_THREADS + threadIdx.x;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
    if (t < 2 * k.g.Vh) {
        const int p = t >= k.g.Vh ? 1 : 0, i = t - p * k.g.Vh;
        int x[4];
        cb_to_coords(k.g, p, i, x);
#pragma unroll 1
        for (int kind = 0; kind < (EXT ? 2 : 3); kind++) {
            double qk = 0.0;
#pragma unroll 1
            for (int pr = 0; pr < 3; pr++) {
                cd Ga[9], Gb[9];
                double ra, rb;
                obs_field<EXT>(Ga, ra, k, x, 0, pr + 1, kind);
                obs_field<EXT>(Gb, rb, k, x, pr == 0 ? 2 : 1, pr == 2 ? 2 : 3, kind);
                const double tab = tr_re(Ga, Gb);
                qk += pr == 1 ? -tab : tab;
                if (kind == 0) v0 += (3.0 - ra) + (3.0 - rb);
                if (kind == 1) v1 -= tr_re(Ga, Ga) + tr_re(Gb, Gb);
            }
            if (kind == 0) v2 = qk;
            else if (kind == 1) v3 = qk;
            else v4 = qk;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v0 += __shfl_down(v0, o, 64); v1 += __shfl_down(v1, o, 64); v2 += __shfl_down(v2, o, 64);
        v3 += __shfl_down(v3, o, 64); v4 += __shfl_down(v4, o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = v0; red[1][w] = v1; red[2][w] = v2; red[3][w] = v3; red[4][w] = v4; }
    __syncthreads();
    if (threadIdx.x < FLOW_RAW) k.partial[(size_t)threadIdx.x * k.nblk + blockIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1];
}

// out[j] = sum over the blocks of partial[j][.], in a fixed order (strided per thread, then a tree)
__global__ __launch_bounds__(256) void flow_obs_final_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ out) {
    __shared__ double s[256];
    for (int j = 0; j < FLOW_RAW; j++) {
        double a = 0.0;
        for (int b = threadIdx.x; b < nblk; b += 256) a += partial[(size_t)j * nblk + b];
        s[threadIdx.x] = a;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[j] = s[0];
        __syncthreads();
    }
}

static int flow_tab_reserve(lqcd_ctx_s* c, size_t n) {
    if (c->flow_tab_n >= n) return LQCD_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)hipFree(c->flow_tab);
    c->flow_tab = nullptr; c->flow_tab_n = 0;
    HIPCHK(hipMalloc((void**)&c->flow_tab, n * sizeof(double)));
    c->flow_tab_n = n;
    return LQCD_OK;
}

// the raw sums of the whole lattice into d_out[0 .. FLOW_RAW) on the device (summed over the ranks); nothing is synchronised with the host
static int obs_enqueue(lqcd_gauge_s* U, double* d_out) {
    lqcd_ctx_s* c = U->ctx;
    ObsArgs k;
    k.g = c->geom;
    k.U = U->data;
    k.ext = nullptr;
    for (int j = 0; j < 4; j++) k.E[j] = 0;
    k.en = 0;
    const int nb = (2 * c->geom.Vh + FLOW_OBS_THREADS - 1) / FLOW_OBS_THREADS;
    if (c->flow_partial_n < (size_t)FLOW_RAW * nb) {
        HIPCHK(hipStreamSynchronize(c->stream));
        (void)hipFree(c->flow_partial);
        c->flow_partial = nullptr; c->flow_partial_n = 0;
        HIPCHK(hipMalloc((void**)&c->flow_partial, (size_t)FLOW_RAW * nb * sizeof(double)));
        c->flow_partial_n = (size_t)FLOW_RAW * nb;
    }
    k.partial = c->flow_partial;
    k.nblk = nb;
    if (any_partitioned(c)) {
        ARGCHK(c->local_peers.empty(), "flow observables: this context belongs to an in-process PE grid");
        LQCHK(gauge_ext_links(c, U, &k.ext, k.E, &k.en));
        hipLaunchKernelGGL(flow_obs_kernel<true>, dim3(nb), dim3(FLOW_OBS_THREADS), 0, c->stream, k);
    } else {
        hipLaunchKernelGGL(flow_obs_kernel<false>, dim3(nb), dim3(FLOW_OBS_THREADS), 0, c->stream, k);
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(flow_obs_final_kernel, dim3(1), dim3(256), 0, c->stream, c->flow_partial, nb, d_out);
    HIPCHK(hipGetLastError());
    if (c->has_comm) LQCHK(comm_allreduce(c, d_out, FLOW_RAW));
    return LQCD_OK;
}

static void obs_finish(lqcd_ctx_s* c, const double* raw, double* obs) {
    const double V = (double)c->gL[0] * c->gL[1] * c->gL[2] * c->gL[3];
    const double qn = -1.0 / (4.0 * M_PI * M_PI);
    obs[0] = 1.0 - raw[0] / (18.0 * V);
    obs[1] = 2.0 * raw[0] / V;
    obs[2] = raw[1] / V;
    obs[3] = qn * raw[2];
    obs[4] = qn * raw[3];
    const double qrect = 2.0 * qn * raw[4];
    obs[5] = any_partitioned(c) ? std::numeric_limits<double>::quiet_NaN() : (5.0 / 3.0) * obs[4] - qrect / 12.0;
}

// accumulator, projection flag and the link path of this flow call (two-row loads when the links are on the group and every stage projects them back)
static int flow_prepare(lqcd_gauge_s* U, double eps, size_t tab_doubles, bool& two_rows) {
    lqcd_ctx_s* c = U->ctx;
    HIPCHK(hipSetDevice(c->device));
    if (!c->flow_x) {
        HIPCHK(hipMalloc((void**)&c->flow_x, U->elems * sizeof(double2)));
        HIPCHK(hipMemsetAsync(c->flow_x, 0, U->elems * sizeof(double2), c->stream));
    }
    LQCHK(flow_tab_reserve(c, tab_doubles));
    HIPCHK(hipMemsetAsync(c->flow_tab, 0, sizeof(double), c->stream));      // word 0: "some link was not projected"
    // The link path of the whole call is fixed here, from the links at entry; the projection flag is read once, at the end (no host synchronisation per
    // step).  Assumption: when the links enter on the group, every stage leaves them there -- exp(X) of a traceless anti-Hermitian X is unitary to
    // rounding (exp_m3: <= 6e-16 for |X| < 2, the Horner form beyond), so the projection of md_reunitarize (deviation <= 1e-13) takes every link.  That is
    // held to step sizes |eps| <= FLOW_TWO_ROW_EPS, where |X| of a stage stays a few units even on a hot start; a larger eps takes the three-row loads.
    // If a link were ever left unprojected, the flag keeps unitary_version behind and the next call takes the three-row loads.
    two_rows = c->tun.staple_recon && c->tun.md_reunitarize && U->unitary_version == U->version && std::fabs(eps) <= FLOW_TWO_ROW_EPS;
    return LQCD_OK;
}
static int flow_rk3_step(lqcd_gauge_s* U, double eps, bool two_rows) {
    lqcd_ctx_s* c = U->ctx;
    unsigned* flag = reinterpret_cast<unsigned*>(c->flow_tab);
    LQCHK(flow_stage(U, c->flow_x, 0.0, 0.25 * eps, false, flag, two_rows));
    LQCHK(flow_stage(U, c->flow_x, -17.0 / 9.0, (8.0 / 9.0) * eps, true, flag, two_rows));
    LQCHK(flow_stage(U, c->flow_x, -1.0, 0.75 * eps, true, flag, two_rows));
    return LQCD_OK;
}
static void flow_done(lqcd_gauge_s* U, const double* word0) {
    unsigned notproj;
    std::memcpy(&notproj, word0, sizeof(unsigned));
    if (U->ctx->tun.md_reunitarize && !notproj) U->unitary_version = U->version;      // every link was projected: the field is on the group to rounding
}
static int flow_args(lqcd_gauge_t V, const char* who) {
    if (!V || !V->ctx) { set_error(std::string(who) + ": null gauge field"); return LQCD_ERR_ARG; }
    if (!V->ctx->local_peers.empty()) { set_error(std::string(who) + ": this context belongs to an in-process PE grid"); return LQCD_ERR_ARG; }
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

// flow!(Usmr, gradientflow) (lqcd.jl:99,153) with Nflow = nsteps: nsteps RK3 steps of size eps, in place
extern "C" int lqcd_gradient_flow(lqcd_gauge_t V, double eps, int nsteps) {
    LQCHK(links_flush_of(V));
    LQCHK(flow_args(V, "lqcd_gradient_flow"));
    ARGCHK(nsteps >= 0 && std::isfinite(eps), "lqcd_gradient_flow: nsteps >= 0 and a finite eps");
    if (nsteps == 0) return LQCD_OK;
    lqcd_ctx_s* c = V->ctx;
    bool two_rows;
    LQCHK(flow_prepare(V, eps, 1, two_rows));
    for (int s = 0; s < nsteps; s++) LQCHK(flow_rk3_step(V, eps, two_rows));
    double word0 = 0.0;
    HIPCHK(hipMemcpyAsync(&word0, c->flow_tab, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->has_comm) LQCHK(comm_check(c));
    flow_done(V, &word0);
    return LQCD_OK;
}

// Energy_density / Topological_charge (lqcd.jl:149-164) of the links as they are: obs = p, E_plaq, E_clov, Q_plaq, Q_clov, Q_impr
extern "C" int lqcd_gauge_flow_observables(lqcd_gauge_t V, double obs[LQCD_FLOW_NOBS]) {
    LQCHK(links_flush_of(V));
    LQCHK(flow_args(V, "lqcd_gauge_flow_observables"));
    ARGCHK(obs, "lqcd_gauge_flow_observables: null obs");
    lqcd_ctx_s* c = V->ctx;
    HIPCHK(hipSetDevice(c->device));
    LQCHK(flow_tab_reserve(c, 1 + FLOW_RAW));
    LQCHK(obs_enqueue(V, c->flow_tab + 1));
    double raw[FLOW_RAW];
    HIPCHK(hipMemcpyAsync(raw, c->flow_tab + 1, sizeof raw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->has_comm) LQCHK(comm_check(c));
    obs_finish(c, raw, obs);
    return LQCD_OK;
}

// the driver's whole gradient-flow schedule (lqcd.jl:149-164) resident: nsteps steps, the observables after every `every`-th; table = nsteps / every rows
// [t, p, E_plaq, E_clov, Q_plaq, Q_clov, Q_impr].  One device-to-host copy, at the end
extern "C" int lqcd_gradient_flow_measure(lqcd_gauge_t V, double eps, int nsteps, int every, double* table) {
    LQCHK(links_flush_of(V));
    LQCHK(flow_args(V, "lqcd_gradient_flow_measure"));
    ARGCHK(nsteps >= 0 && every >= 1 && std::isfinite(eps), "lqcd_gradient_flow_measure: nsteps >= 0, every >= 1 and a finite eps");
    const int nrows = nsteps / every;
    ARGCHK(table || nrows == 0, "lqcd_gradient_flow_measure: null table");
    if (nsteps == 0) return LQCD_OK;
    lqcd_ctx_s* c = V->ctx;
    bool two_rows;
    LQCHK(flow_prepare(V, eps, 1 + (size_t)FLOW_RAW * nrows, two_rows));
    int row = 0;
    for (int s = 1; s <= nsteps; s++) {
        LQCHK(flow_rk3_step(V, eps, two_rows));
        if (s % every == 0) LQCHK(obs_enqueue(V, c->flow_tab + 1 + (size_t)FLOW_RAW * row++));
    }
    std::vector<double> h(1 + (size_t)FLOW_RAW * nrows);
    HIPCHK(hipMemcpyAsync(h.data(), c->flow_tab, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->has_comm) LQCHK(comm_check(c));
    flow_done(V, h.data());
    for (int r = 0; r < nrows; r++) {
        table[(size_t)r * (1 + LQCD_FLOW_NOBS)] = (double)((r + 1) * every) * eps;
        obs_finish(c, h.data() + 1 + (size_t)FLOW_RAW * r, table + (size_t)r * (1 + LQCD_FLOW_NOBS) + 1);
    }
    return LQCD_OK;
}
