// heatbath.hip -- quenched SU(3) heatbath and overrelaxation sweeps on the device: the reference's third update method, "Heatbath"
// (src/updates/AbstractUpdate.jl:59-108, src/updates/heatbath.jl:1-44: Heatbath(U, beta; ITERATION_MAX), heatbath!(U, hb), overrelaxation!(U, hb)).
//
// Contract (tests/heatbath_numpy.py restates it; directions 0..3 = x, y, z, t):
//   action      S_g = -(beta/3) sum_plaq Re tr U_p (lqcd_gauge_action, the staple force).  Staple sum A_mu(x) = the six staples of lqcd_link_staple without
//               its beta/2: upper U_nu(x+mu) U_mu(x+nu)^+ U_nu(x)^+, lower U_nu(x-nu+mu)^+ U_mu(x-nu)^+ U_nu(x-nu); Re tr(U_mu(x) A_mu(x)) is the sum of
//               the six plaquettes through the link, so the link's weight is exp((beta/3) Re tr(U A)).
//   sweep       for mu = 0..3, parity 0 (even) then 1 (odd): every link U_mu(x) of that parity, in place, one launch per (mu, parity).
//               In-place is exact: launch (mu, p) writes U_mu at parity p only and reads U_mu only at parity 1 - p (x +- nu, x - nu + mu: the
//               other parity) plus the other directions -- no lane reads a link another lane of the launch writes, whatever order lanes run in.
//   heatbath    Cabibbo-Marinari over the SU(2) subgroups (0,1), (0,2), (1,2), in that order.  W = U A; of the 2x2 block w of W (rows / columns i, j)
//               take the quaternion part a = (Re(w00 + w11), Im(w01 + w10), Re(w01 - w10), Im(w00 - w11)) / 2 <-> a0 + i a.sigma, k = |a|, v = a / k
//               (v = 1 when k = 0).  Draw y in SU(2) with density exp(alpha y0) dHaar(y), alpha = (2 beta / 3) k, set R = y v^+ and U <- R U, W <- R W
//               (rows i, j; R = [[r0 + i r3, r2 + i r1], [-r2 + i r1, r0 - i r3]]).  Quaternion product (p q)_0 = p0 q0 - p.q,
//               (p q)_vec = p0 q + q0 p - p x q.
//   y0          alpha == 0 (beta = 0, the Haar limit): y0 = 2 u0 - 1, accepted when u1^2 <= 1 - y0^2
//               0 < alpha < HB_KP_ALPHA (Creutz): y0 = 1 + log1p((1 - u0) expm1(-2 alpha)) / alpha, accepted when u1^2 <= 1 - y0^2
//               alpha >= HB_KP_ALPHA (Kennedy-Pendleton): s = -(log u0 + cos^2(2 pi u1) log u2) / (2 alpha), accepted when u3^2 <= 1 - s; y0 = 1 - 2 s
//   direction   z = 2 d0 - 1, phi = 2 pi d1: (y1, y2, y3) = sqrt(1 - y0^2) (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z)
//   overrelax   the same order with R = (v^+)^2, the microcanonical reflection: Re tr(U A) is kept, no random numbers, no beta; k = 0 leaves the subgroup alone
//   projection  after its three subgroups the link goes back onto SU(3) by the rule of lqcd_gauge_reunitarize (Gram-Schmidt on rows 0, 1, row 2 =
//               conj(row 0 x row 1); gauge_staple.h reunitarize_m3), so the field is on the group (unitary_version = version) after every call
//   draws       key = rng_key(seed ^ HB_SALT, global site, 4 sweep + mu, subgroup), draw j = u01(splitmix64(key + j)).  Trial t = 0, 1, ... of the y0 sampler
//               takes j = 4t .. 4t + 3 (u0 .. u3; the Creutz and Haar branches use the first two), the direction d0, d1 = j = HB_DIR_J, HB_DIR_J + 1.
//               sweep = first_sweep + i for the i-th heatbath sweep of a call (overrelaxation draws nothing): a run split into calls gives the bits of one
//               call, and no draw depends on launch geometry, partitioning or when a lane retires.
//   cap         itmax trials per draw (the reference's ITERATION_MAX).  A draw that runs out leaves its subgroup alone and adds to a device counter; the call
//               then returns LQCD_ERR_NOT_CONVERGED with the count in lqcd_last_error().  The links stay on the group.
// Partitioned lattices (RCCL or the peer backend): before every (mu, parity) launch the forward ghost links and the received lower staples are refreshed
// by the staple force's exchange (staple.hip staple_halo_args), 8 refreshes per sweep.  An in-process PE grid answers LQCD_ERR_UNSUPPORTED.
#include "lqcd_internal.h"
#include "gauge_staple.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace lqcd {

constexpr uint64_t HB_SALT = 0x6865617462617468ull;     // "heatbath"
constexpr uint64_t HB_DIR_J = 1ull << 40;               // first draw of the direction, past every trial block
constexpr double HB_KP_ALPHA = 2.0;                     // Kennedy-Pendleton at and above, Creutz below
constexpr int HB_THREADS = 256;

struct HBArgs {
    GFArgs s;               // geometry, links (read side), forward ghosts and received lower staples
    double2* U;             // the links, written in place
    int mu, p;
    int itmax;
    double alpha_k;         // 2 beta / 3: alpha = alpha_k * k
    uint64_t seed, sweep;   // seed ^ HB_SALT, absolute sweep number
    unsigned* capped;       // draws that ran out of trials
};

// y0 with density ~ sqrt(1 - y0^2) exp(alpha y0).  The loop is per lane: the wave runs it while any lane still has to accept and lanes that accepted sit
// predicated off; a lane's draws depend on its own trial index only.
__device__ __forceinline__ bool hb_y0(double& y0, double alpha, uint64_t key, int itmax) {
    const bool kp = alpha >= HB_KP_ALPHA;
    const double em = kp ? 0.0 : expm1(-2.0 * alpha), ia = alpha > 0.0 ? 1.0 / alpha : 0.0;
    for (int t = 0; t < itmax; t++) {
        const uint64_t j = key + 4 * (uint64_t)t;
        const double u0 = u01(splitmix64(j)), u1 = u01(splitmix64(j + 1));
        if (kp) {
            const double u2 = u01(splitmix64(j + 2)), u3 = u01(splitmix64(j + 3));
            const double cs = cos(6.283185307179586 * u1);
            const double s = -(log(u0) + cs * cs * log(u2)) * (0.5 * ia);
            if (u3 * u3 <= 1.0 - s) { y0 = 1.0 - 2.0 * s; return true; }
        } else {
            const double y = alpha == 0.0 ? 2.0 * u0 - 1.0 : 1.0 + log1p((1.0 - u0) * em) * ia;
            if (u1 * u1 <= 1.0 - y * y) { y0 = y; return true; }
        }
    }
    return false;
}

// R (quaternion r) applied to rows I, J of M
template <int I, int J>
__device__ __forceinline__ void su2_rows(cd (&M)[9], double r0, double r1, double r2, double r3) {
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const cd x = M[I * 3 + b], y = M[J * 3 + b];
        M[I * 3 + b] = cmul(mk(r0, r3), x) + cmul(mk(r2, r1), y);
        M[J * 3 + b] = cmul(mk(-r2, r1), x) + cmul(mk(r0, -r3), y);
    }
}

// one subgroup (I, J) of one link: heatbath (OR = false) or overrelaxation; W = U A is kept current for the subgroups after it
template <bool OR, int I, int J, int SG>
__device__ __forceinline__ void su2_update(cd (&U)[9], cd (&W)[9], const HBArgs& h, uint64_t site) {
    const cd w00 = W[I * 3 + I], w01 = W[I * 3 + J], w10 = W[J * 3 + I], w11 = W[J * 3 + J];
    const double a0 = 0.5 * (w00.re + w11.re), a1 = 0.5 * (w01.im + w10.im), a2 = 0.5 * (w01.re - w10.re), a3 = 0.5 * (w00.im - w11.im);
    const double k = sqrt(a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3);
    double r0, r1, r2, r3;
    if constexpr (OR) {
        if (k == 0.0) return;
        const double ik = 1.0 / k, v0 = a0 * ik, v1 = a1 * ik, v2 = a2 * ik, v3 = a3 * ik;
        r0 = v0 * v0 - (v1 * v1 + v2 * v2 + v3 * v3);
        r1 = -2.0 * v0 * v1; r2 = -2.0 * v0 * v2; r3 = -2.0 * v0 * v3;
    } else {
        const uint64_t key = rng_key(h.seed, site, 4 * h.sweep + (uint64_t)h.mu, SG);
        double y0;
        if (!hb_y0(y0, h.alpha_k * k, key, h.itmax)) { atomicAdd(h.capped, 1u); return; }
        const double z = 2.0 * u01(splitmix64(key + HB_DIR_J)) - 1.0, phi = 6.283185307179586 * u01(splitmix64(key + HB_DIR_J + 1));
        const double ry = sqrt(fmax(0.0, 1.0 - y0 * y0)), rz = sqrt(fmax(0.0, 1.0 - z * z));
        double sp, cp;
        sincos(phi, &sp, &cp);
        const double y1 = ry * rz * cp, y2 = ry * rz * sp, y3 = ry * z;
        double v0 = 1.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
        if (k > 0.0) {
            const double ik = 1.0 / k;
            v0 = a0 * ik; v1 = a1 * ik; v2 = a2 * ik; v3 = a3 * ik;
        }
        // R = y v^+ = (y0 v0 + y.v,  v0 y - y0 v + y x v)
        r0 = y0 * v0 + (y1 * v1 + y2 * v2 + y3 * v3);
        r1 = v0 * y1 - y0 * v1 + (y2 * v3 - y3 * v2);
        r2 = v0 * y2 - y0 * v2 + (y3 * v1 - y1 * v3);
        r3 = v0 * y3 - y0 * v3 + (y1 * v2 - y2 * v1);
    }
    su2_rows<I, J>(U, r0, r1, r2, r3);
    if constexpr (SG < 2) su2_rows<I, J>(W, r0, r1, r2, r3);
}

// one (mu, parity) launch: lane = site of parity p; run-time direction (the partitioned form of staple.hip gauge_force_kernel_part)
template <bool OR, bool PART>
__global__ __launch_bounds__(HB_THREADS) void heatbath_kernel(HBArgs h) {
    const GFArgs& k = h.s;
    const Geom& g = k.g;
    const int p = h.p, mu = h.mu, i = blockIdx.x * HB_THREADS + threadIdx.x;
    if (i >= g.Vh) return;
    const int Gs = glink_stride(g);
    int c[4];
    cb_to_coords(g, p, i, c);
    cd A[9];
#pragma unroll
    for (int e = 0; e < 9; e++) A[e] = mk(0.0, 0.0);
#pragma unroll 1
    for (int nu = 0; nu < 4; nu++) {
        if (nu == mu) continue;
        cd u1[9], u2[9], u3[9], t1[9], t2[9];
        link_fwd<PART>(u1, k, c, mu, nu);                   // U_nu(x+mu)
        link_fwd<PART>(u2, k, c, nu, mu);                   // U_mu(x+nu)
        load_m3(u3, link_at(g, k.U, c, nu), Gs);
        mm3_nd(t1, u1, u2);
        mm3_nd(t2, t1, u3);
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = A[e] + t2[e];
        if (PART && c[nu] == 0 && g.part[nu]) {             // x - nu lives on the -nu neighbour: its lower staple arrived with the exchange
            const int Fh = face_half_sites(g, nu), f = coords_to_face(g, nu, c);
            const double2* b = k.wrecv[nu] + ((size_t)((1 - p) * 4 + mu) * 9) * Fh + f;
#pragma unroll
            for (int e = 0; e < 9; e++) t2[e] = ld(b + (size_t)e * Fh);
        } else {
            int m[4] = {c[0], c[1], c[2], c[3]};
            shift(m, g, nu, -1);
            lower_staple_at<PART>(t2, k, m, mu, nu);
        }
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = A[e] + t2[e];
    }
    double2* o = h.U + glink_off(g, p, mu, i);
    cd U[9], W[9];
    load_m3(U, o, Gs);
    mm3(W, U, A);
    const uint64_t site = (uint64_t)(c[0] + g.origin[0]) +
                          (uint64_t)g.gL[0] * ((uint64_t)(c[1] + g.origin[1]) + (uint64_t)g.gL[1] * ((uint64_t)(c[2] + g.origin[2]) + (uint64_t)g.gL[2] * (uint64_t)(c[3] + g.origin[3])));
    su2_update<OR, 0, 1, 0>(U, W, h, site);
    su2_update<OR, 0, 2, 1>(U, W, h, site);
    su2_update<OR, 1, 2, 2>(U, W, h, site);
    reunitarize_m3(U);
#pragma unroll
    for (int e = 0; e < 9; e++) st(o + (size_t)e * Gs, U[e]);
}

static int hb_tab_reserve(lqcd_ctx_s* c, size_t n) {
    if (c->hb_tab_n >= n) return LQCD_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)hipFree(c->hb_tab);
    c->hb_tab = nullptr; c->hb_tab_n = 0;
    HIPCHK(hipMalloc((void**)&c->hb_tab, n * sizeof(double)));
    c->hb_tab_n = n;
    return LQCD_OK;
}

// one sweep: 4 directions x 2 parities, in place
static int hb_sweep(lqcd_gauge_s* U, bool over, double beta, int itmax, uint64_t seed, uint64_t sweep) {
    lqcd_ctx_s* c = U->ctx;
    const bool part = any_partitioned(c);
    HBArgs h;
    h.U = U->data;
    h.itmax = itmax;
    h.alpha_k = 2.0 * beta / 3.0;
    h.seed = seed ^ HB_SALT;
    h.sweep = sweep;
    h.capped = reinterpret_cast<unsigned*>(c->hb_tab);
    const dim3 grid((c->geom.Vh + HB_THREADS - 1) / HB_THREADS);
    if (!part) LQCHK(staple_halo_args(U, h.s));
    for (int mu = 0; mu < 4; mu++)
        for (int p = 0; p < 2; p++) {
            if (part) LQCHK(staple_halo_args(U, h.s));      // the ghosts and lower staples of the links as the previous launch left them
            h.mu = mu; h.p = p;
            if (over && part) hipLaunchKernelGGL((heatbath_kernel<true, true>), grid, dim3(HB_THREADS), 0, c->stream, h);
            else if (over) hipLaunchKernelGGL((heatbath_kernel<true, false>), grid, dim3(HB_THREADS), 0, c->stream, h);
            else if (part) hipLaunchKernelGGL((heatbath_kernel<false, true>), grid, dim3(HB_THREADS), 0, c->stream, h);
            else hipLaunchKernelGGL((heatbath_kernel<false, false>), grid, dim3(HB_THREADS), 0, c->stream, h);
            HIPCHK(hipGetLastError());
        }
    return LQCD_OK;
}

// the local plaquette sum of the links as they are into d_sum (device), summed over the ranks on a partitioned lattice
static int hb_plaquette(lqcd_gauge_s* U, double* d_sum) {
    lqcd_ctx_s* c = U->ctx;
    if (!any_partitioned(c)) return plaquette_local_sum_device(U, nullptr, d_sum);
    LQCHK(gauge_halo_links(U));
    LQCHK(plaquette_local_sum_device(U, c->gf_ghost, d_sum));
    return comm_allreduce(c, d_sum, 1);
}

static int hb_args(lqcd_gauge_t U, const char* who) {
    if (!U || !U->ctx) { set_error(std::string(who) + ": null gauge field"); return LQCD_ERR_ARG; }
    return LQCD_OK;
}
static int hb_grid_check(lqcd_gauge_t U, const char* who) {
    if (!U->ctx->local_peers.empty()) {
        set_error(std::string(who) + ": this context belongs to an in-process PE grid");
        return LQCD_ERR_UNSUPPORTED;
    }
    return LQCD_OK;
}

// nsweeps x (one heatbath sweep (heat) + nor OR sweeps); plaq (may be null): the plaquette after every heatbath + OR block, slot i of the device table.
// Word 0 of the table counts the draws that ran out of trials.  One device-to-host copy at the end.
static int hb_run(lqcd_gauge_s* U, const char* who, bool heat, double beta, int nsweeps, int nor, int itmax, uint64_t seed, uint64_t first_sweep,
                  double* plaq) {
    lqcd_ctx_s* c = U->ctx;
    HIPCHK(hipSetDevice(c->device));
    const size_t ntab = 1 + (plaq ? (size_t)nsweeps : 0);
    LQCHK(hb_tab_reserve(c, ntab));
    HIPCHK(hipMemsetAsync(c->hb_tab, 0, sizeof(double), c->stream));
    for (int s = 0; s < nsweeps; s++) {
        if (heat) LQCHK(hb_sweep(U, false, beta, itmax, seed, first_sweep + (uint64_t)s));
        for (int r = 0; r < nor; r++) LQCHK(hb_sweep(U, true, 0.0, 1, 0, 0));
        if (plaq) LQCHK(hb_plaquette(U, c->hb_tab + 1 + s));
    }
    U->version++;
    U->unitary_version = U->version;      // every link was projected onto SU(3) by its last update
    std::vector<double> hb(ntab);
    HIPCHK(hipMemcpyAsync(hb.data(), c->hb_tab, ntab * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->has_comm) LQCHK(comm_check(c));
    unsigned capped;
    std::memcpy(&capped, hb.data(), sizeof(unsigned));
    const double V = (double)c->gL[0] * c->gL[1] * c->gL[2] * c->gL[3];
    for (int s = 0; plaq && s < nsweeps; s++) plaq[s] = hb[1 + s] / (6.0 * V * 3.0);      // the normalisation of lqcd_gauge_plaquette
    double ncap = (double)capped;
    if (c->has_comm) LQCHK(allreduce_host(c, &ncap, 1));
    if (ncap > 0.0) {
        set_error(std::string(who) + ": " + std::to_string((long long)ncap) + " SU(2) draws ran out of itmax trials (their subgroups were left unchanged)");
        return LQCD_ERR_NOT_CONVERGED;
    }
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

// heatbath!(U, hb) + numOR x overrelaxation!(U, hb) (heatbath.jl:35-43), nsweeps times
extern "C" int lqcd_gauge_heatbath(lqcd_gauge_t U, double beta, int nsweeps, int nor, int itmax, uint64_t seed, uint64_t first_sweep) {
    LQCHK(hb_args(U, "lqcd_gauge_heatbath"));
    LQCHK(links_flush_of(U));
    ARGCHK(beta >= 0.0 && std::isfinite(beta) && nsweeps >= 0 && nor >= 0 && itmax >= 1,
           "lqcd_gauge_heatbath: beta >= 0 (finite), nsweeps >= 0, nor >= 0 and itmax >= 1");
    LQCHK(hb_grid_check(U, "lqcd_gauge_heatbath"));
    if (nsweeps == 0) return LQCD_OK;
    return hb_run(U, "lqcd_gauge_heatbath", true, beta, nsweeps, nor, itmax, seed, first_sweep, nullptr);
}

// overrelaxation!(U, hb): nsweeps microcanonical sweeps (no random numbers, independent of beta)
extern "C" int lqcd_gauge_overrelax(lqcd_gauge_t U, int nsweeps) {
    LQCHK(hb_args(U, "lqcd_gauge_overrelax"));
    LQCHK(links_flush_of(U));
    ARGCHK(nsweeps >= 0, "lqcd_gauge_overrelax: nsweeps >= 0");
    LQCHK(hb_grid_check(U, "lqcd_gauge_overrelax"));
    if (nsweeps == 0) return LQCD_OK;
    return hb_run(U, "lqcd_gauge_overrelax", false, 0.0, 1, nsweeps, 1, 0, 0, nullptr);
}

// lqcd_gauge_heatbath with the plaquette after every heatbath + OR block: plaq[i] equals lqcd_gauge_plaquette of the links after block i (bit for bit on a
// single domain: the same block partials added in the same order, on the device)
extern "C" int lqcd_gauge_heatbath_measure(lqcd_gauge_t U, double beta, int nsweeps, int nor, int itmax, uint64_t seed, uint64_t first_sweep, double* plaq) {
    LQCHK(hb_args(U, "lqcd_gauge_heatbath_measure"));
    LQCHK(links_flush_of(U));
    ARGCHK(beta >= 0.0 && std::isfinite(beta) && nsweeps >= 0 && nor >= 0 && itmax >= 1 && plaq,
           "lqcd_gauge_heatbath_measure: beta >= 0 (finite), nsweeps >= 0, nor >= 0, itmax >= 1 and a plaq array");
    LQCHK(hb_grid_check(U, "lqcd_gauge_heatbath_measure"));
    if (nsweeps == 0) return LQCD_OK;
    return hb_run(U, "lqcd_gauge_heatbath_measure", true, beta, nsweeps, nor, itmax, seed, first_sweep, plaq);
}
