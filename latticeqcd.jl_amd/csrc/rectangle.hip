// rectangle.hip -- the plaquette + rectangle gauge action (tree-level Symanzik / Luscher-Weisz, Iwasaki, DBW2: the reference's GaugeAction with couplingcoeff on
// [plaqloops, rectloops], examples/param_symanzik_improved_hb.jl) on the gauge side of the MD step: mean rectangle, action, force field, the momentum update fused
// onto the force, and the single-direction staple sum of calc_dSdUmu!.  Single domain only; conventions beside those of md.hip:
//   S_g = -(1/3) [ beta_plaq sum_plaq Re tr U_p + beta_rect sum_rect Re tr U_r ], the sums over the 6 V plaquettes and the 12 V rectangles (1x2 and 2x1, every plane,
//   every corner).  Luscher-Weisz: beta_plaq = 5 beta / 3, beta_rect = -beta / 12.  Iwasaki / DBW2: beta_plaq = (1 - 8 c1) beta, beta_rect = c1 beta, c1 = -0.331 / -1.4088.
//   Rectangle staples of the link (n, mu): 18, six per nu != mu -- long side along mu with the link as its first or its second half, above and below (4), long side
//   along nu, above and below (2) -- each the ordered product of the other five links from n + mu back to n, so that tr(U_mu(n) staple) is the loop (the orientation
//   of lower_staple_at, gauge_staple.h).
//   G_mu(n) = -(1/6) U_mu(n) [ beta_plaq (six plaquette staples) + beta_rect (eighteen rectangle staples) ]; by linearity it obeys the rule of every force field,
//   dS/d eps [U -> exp(i eps T) U] = -2 Im tr(T G), hence dP/dtau = TA(G).
// An extent of 2: a 2-long side closes on itself through the periodic wrap (n + 2 mu = n).  The sweep and the sum take every neighbour by wrapped coordinates, so
// such a lattice is computed, not refused: the 12 V rectangles are still 12 V distinct (corner, orientation) pairs, and a link that occurs twice in one loop gets
// both staples (the product rule) -- tested against the restatement and by finite differences on (4,4,2,2).
// Refused (LQCD_ERR_UNSUPPORTED): a partitioned lattice and an in-process PE grid -- the rectangles need a halo of depth 2 (the reason Q_impr is NaN there, flow.hip).
// Not here: heat bath / overrelaxation (the (mu, parity) colouring of heatbath.hip is invalid: a rectangle couples U_mu(n) to U_mu(n + mu), U_mu(n +- nu), U_mu(n + 2 nu)),
// the one-sweep P + U form, recorder fusion of the per-direction triple, the Symanzik flow.
//
// The staple sweep per plane (mu, nu), with A1 = U_nu(n+mu), B = U_mu(n+nu), C = U_nu(n) above and D = U_nu(n+mu-nu), E = U_mu(n-nu), F = U_nu(n-nu) below:
//   above:  A1 [ (wp B^+ + wr X5) C^+ ]  +  wr A1 [ B^+ X3 ]  +  wr [ X1 B^+ ] C^+       X5 = U_nu(n+mu+nu) U_mu(n+2nu)^+ U_nu(n+nu)^+     (long side along nu)
//                                                                                       X3 = U_mu(n-mu+nu)^+ U_nu(n-mu)^+ U_mu(n-mu)      (link = second half)
//                                                                                       X1 = U_mu(n+mu) U_nu(n+2mu) U_mu(n+mu+nu)^+       (link = first half)
//   below:  D^+ [ (wp E^+ + wr Y6) F ]   +  wr D^+ [ E^+ Y4 ]  +  wr [ Y2 E^+ ] F        Y6 = U_nu(n+mu-2nu)^+ U_mu(n-2nu)^+ U_nu(n-2nu)
//                                                                                       Y4 = U_mu(n-mu-nu)^+ U_nu(n-mu-nu) U_mu(n-mu)
//                                                                                       Y2 = U_mu(n+mu) U_nu(n+2mu-nu)^+ U_mu(n+mu-nu)^+
// The plaquette staple rides inside the product of the long-side-along-nu rectangle (its corner links A1, C / D, F are that rectangle's outer links), so a plane is
// six chains of four products, the last one added straight into the staple sum: 24 products per plane, 72 + 1 per link, where the eighteen five-link chains and the
// six plaquette staples one by one take 84 + 12.  Each chain holds the sum and three matrices; the corner links B, A1, C (E, D, F) are asked for once per chain that
// ends on them -- 32 loads per plane (96 + 1 per link), the repeats hits of the same 1 KiB lines -- instead of being held across the chains: held, the sweep took
// 256 + 16 registers and one wave per SIMD.
#include "lqcd_internal.h"
#include "gauge_staple.h"

namespace lqcd {

struct RectArgs {
    Geom g;
    const double2* U;
    double2* out;
    double wp, wr;           // weights of the plaquette and of the rectangle staples in the staple sum
    double coef, factor;     // G = coef U_mu(n) (staple sum); MODE 1: out += factor TA(G)
    BlockMap bm;
    int mu_only, mu_out;     // MODE 2: direction mu_only, the staple sum goes to slot mu_out of `out`
    double* partial;         // rectangle sum: one partial per workgroup
};

// A += w X Y,  A += w X^+ Y,  A += w X Y^+
__device__ __forceinline__ void macc3(cd (&A)[9], double w, const cd (&X)[9], const cd (&Y)[9]) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            cd t = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) cfma(t, X[a * 3 + k], Y[k * 3 + b]);
            A[a * 3 + b] = mk(fma(w, t.re, A[a * 3 + b].re), fma(w, t.im, A[a * 3 + b].im));
        }
}
__device__ __forceinline__ void macc3_dn(cd (&A)[9], double w, const cd (&X)[9], const cd (&Y)[9]) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            cd t = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) cfma_conj(t, X[k * 3 + a], Y[k * 3 + b]);
            A[a * 3 + b] = mk(fma(w, t.re, A[a * 3 + b].re), fma(w, t.im, A[a * 3 + b].im));
        }
}
__device__ __forceinline__ void macc3_nd(cd (&A)[9], double w, const cd (&X)[9], const cd (&Y)[9]) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            cd t = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) cfma_conj(t, Y[b * 3 + k], X[a * 3 + k]);
            A[a * 3 + b] = mk(fma(w, t.re, A[a * 3 + b].re), fma(w, t.im, A[a * 3 + b].im));
        }
}
// M <- wp B^+ + wr M
__device__ __forceinline__ void mix_dag(cd (&M)[9], double wp, const cd (&B)[9], double wr) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) M[a * 3 + b] = mk(fma(wp, B[b * 3 + a].re, wr * M[a * 3 + b].re), fma(-wp, B[b * 3 + a].im, wr * M[a * 3 + b].im));
}

__device__ __forceinline__ int wrap2(int x, int L) {      // x in [-2, L + 2), L >= 2
    if (x >= L) x -= L;
    if (x < 0) x += L;
    return x;
}
// U_dir at n + a mu_hat + b nu_hat (|a|, |b| <= 2, periodic)
template <int MU, int NU, bool R2>
__device__ __forceinline__ void link_off(cd (&u)[9], const RectArgs& k, const int (&c)[4], int a, int b, int dir) {
    int d[4] = {c[0], c[1], c[2], c[3]};
    d[MU] = wrap2(c[MU] + a, k.g.L[MU]);
    d[NU] = wrap2(c[NU] + b, k.g.L[NU]);
    load_u<R2>(u, link_at(k.g, k.U, d, dir), glink_stride(k.g));
}

// the next chain's loads wait for this chain's sum, and are loads of their own (staple.hip staple_plane: without the tie the scheduler hoists the loads of a whole
// direction; with the memory clobber the corner links are loaded again instead of staying live across the chains)
__device__ __forceinline__ void chain_tie(int (&c)[4], cd (&A)[9]) {
    asm volatile("" : "+v"(c[0]), "+v"(A[0].re), "+v"(A[0].im), "+v"(A[4].re), "+v"(A[4].im), "+v"(A[8].re), "+v"(A[8].im) : : "memory");
}

// inside a chain: the next load waits for the product M.  Without these ties the scheduler hoists the loads of a whole chain above its products: 256 VGPRs and
// 20..28 B of scratch per lane at two workgroups per CU, or 256 + 2..6 AGPRs at one -- which ran within 5 % of this form either way (profiles/r18_rect_action.log)
__device__ __forceinline__ void step_tie(int (&c)[4], cd (&M)[9]) {
    asm volatile("" : "+v"(c[0]), "+v"(M[0].re), "+v"(M[4].im), "+v"(M[8].re));
}

// one plane of the staple sum of link (n, MU): A += wp (two plaquette staples) + wr (six rectangle staples); file header
template <int MU, int NU, bool R2>
__device__ __forceinline__ void rect_plane(cd (&A)[9], const RectArgs& k, int (&c)[4]) {
    if constexpr (MU != NU) {
        const double wp = k.wp, wr = k.wr;
#pragma unroll
        for (int s = 1; s >= -1; s -= 2) {      // s = +1: the staples above the link, -1: below
            const int s0 = s > 0 ? 0 : -1;      // the nu offset of the near row of nu links: n / n - nu
            cd x[9], y[9], z[9];
            // the rectangle with its long side along nu, the plaquette staple inside the same product
            link_off<MU, NU, R2>(x, k, c, 1, s > 0 ? 1 : -2, NU);
            link_off<MU, NU, R2>(y, k, c, 0, 2 * s, MU);
            if (s > 0) mm3_nd(z, x, y); else mm3_dd(z, x, y);
            step_tie(c, z);
            link_off<MU, NU, R2>(x, k, c, 0, s > 0 ? 1 : -2, NU);
            if (s > 0) mm3_nd(y, z, x); else mm3(y, z, x);                  // X5 / Y6
            step_tie(c, y);
            link_off<MU, NU, R2>(x, k, c, 0, s, MU);                        // B / E
            mix_dag(y, wp, x, wr);
            link_off<MU, NU, R2>(x, k, c, 0, s0, NU);                       // C / F
            if (s > 0) mm3_nd(z, y, x); else mm3(z, y, x);
            step_tie(c, z);
            link_off<MU, NU, R2>(x, k, c, 1, s0, NU);                       // A1 / D
            if (s > 0) macc3(A, 1.0, x, z); else macc3_dn(A, 1.0, x, z);
            chain_tie(c, A);
            // the link is the second half of the long side: A1 (B^+ X3) / D^+ (E^+ Y4)
            link_off<MU, NU, R2>(x, k, c, -1, s, MU);
            link_off<MU, NU, R2>(y, k, c, -1, s0, NU);
            if (s > 0) mm3_dd(z, x, y); else mm3_dn(z, x, y);
            step_tie(c, z);
            link_off<MU, NU, R2>(x, k, c, -1, 0, MU);
            mm3(y, z, x);                                                   // X3 / Y4
            step_tie(c, y);
            link_off<MU, NU, R2>(x, k, c, 0, s, MU);                        // B / E
            mm3_dn(z, x, y);
            step_tie(c, z);
            link_off<MU, NU, R2>(x, k, c, 1, s0, NU);                       // A1 / D
            if (s > 0) macc3(A, wr, x, z); else macc3_dn(A, wr, x, z);
            chain_tie(c, A);
            // the link is the first half: (X1 B^+) C^+ / (Y2 E^+) F
            link_off<MU, NU, R2>(x, k, c, 1, 0, MU);
            link_off<MU, NU, R2>(y, k, c, 2, s0, NU);
            if (s > 0) mm3(z, x, y); else mm3_nd(z, x, y);
            step_tie(c, z);
            link_off<MU, NU, R2>(x, k, c, 1, s, MU);
            mm3_nd(y, z, x);                                                // X1 / Y2
            step_tie(c, y);
            link_off<MU, NU, R2>(x, k, c, 0, s, MU);                        // B / E
            mm3_nd(z, y, x);
            step_tie(c, z);
            link_off<MU, NU, R2>(x, k, c, 0, s0, NU);                       // C / F
            if (s > 0) macc3_nd(A, wr, z, x); else macc3(A, wr, z, x);
            chain_tie(c, A);
        }
    }
}

template <int MODE, int MU, bool R2>
__device__ __forceinline__ void rect_links(const RectArgs& k, int p, int i) {
    const Geom& g = k.g;
    const int Gs = glink_stride(g);
    int c[4];
    cb_to_coords(g, p, i, c);
    cd A[9];
#pragma unroll
    for (int e = 0; e < 9; e++) A[e] = mk(0.0, 0.0);
    rect_plane<MU, 0, R2>(A, k, c);
    rect_plane<MU, 1, R2>(A, k, c);
    rect_plane<MU, 2, R2>(A, k, c);
    rect_plane<MU, 3, R2>(A, k, c);
    if constexpr (MODE == 2) {
        store_m3(k.out + glink_off(g, p, k.mu_out, i), Gs, A);
        return;
    }
    cd um[9], r[9];
    load_u<R2>(um, k.U + glink_off(g, p, MU, i), Gs);
    mm3(r, um, A);
    double2* o = k.out + glink_off(g, p, MU, i);
    if constexpr (MODE == 0) {
#pragma unroll
        for (int e = 0; e < 9; e++) st(o + (size_t)e * Gs, mk(k.coef * r[e].re, k.coef * r[e].im));
    } else {
        // the TA-upper-triangle contract of lqcd_momentum_add_gauge_force (staple.hip staple_links): the momenta are anti-Hermitian and so is the increment
        cd a[9];
        ta3(a, r, 0.5 * k.coef * k.factor);
        auto addp = [&](auto E) {
            constexpr int e = decltype(E)::value;
            const cd pv = ld(o + (size_t)e * Gs);
            a[e] = mk(pv.re + a[e].re, pv.im + a[e].im);
        };
        addp(std::integral_constant<int, 0>()); addp(std::integral_constant<int, 1>()); addp(std::integral_constant<int, 2>());
        addp(std::integral_constant<int, 4>()); addp(std::integral_constant<int, 5>()); addp(std::integral_constant<int, 8>());
        a[3] = mk(-a[1].re, a[1].im); a[6] = mk(-a[2].re, a[2].im); a[7] = mk(-a[5].re, a[5].im);
        store_m3(o, Gs, a);
    }
}

// workgroup = 64 sites of one parity (a chunk of the chunk-blocked link layout, through the BlockMap of the staple sweep) x 4 waves, wave = mu, dispatched to a
// compile-time direction; MODE 2: 64-thread workgroups, one direction.  Two workgroups per CU (RECT_OCC): 214 (two-row loads) / 250 VGPRs, no scratch.
// MODE 0: out = G.   MODE 1: out (the momenta) += factor TA(G), G never stored.   MODE 2: out[mu_out] = wp (plaquette staples) + wr (rectangle staples) of mu_only.
constexpr int RECT_OCC = 2;
template <int MODE, bool R2>
__global__ __launch_bounds__(256, RECT_OCC) void rect_force_kernel(RectArgs k) {
    int chunk, p;
    block_map(k.bm, blockIdx.x, chunk, p);
    const int i = chunk * 64 + (int)(threadIdx.x & 63);
    const int mu = MODE == 2 ? k.mu_only : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= k.g.Vh) return;
    switch (mu) {
    case 0: rect_links<MODE, 0, R2>(k, p, i); break;
    case 1: rect_links<MODE, 1, R2>(k, p, i); break;
    case 2: rect_links<MODE, 2, R2>(k, p, i); break;
    default: rect_links<MODE, 3, R2>(k, p, i); break;
    }
}

// Re tr of the rectangle with corner c, long side (two links) along a, short side along b
__device__ __forceinline__ double rect_retr(const Geom& g, const double2* __restrict__ U, const int (&c)[4], int a, int b) {
    const int Gs = glink_stride(g);
    int d[4] = {c[0], c[1], c[2], c[3]};
    cd P[9], u[9], t[9];
    load_m3(P, link_at(g, U, d, a), Gs);
    shift(d, g, a, 1);
    load_m3(u, link_at(g, U, d, a), Gs);
    mm3(t, P, u);
    shift(d, g, a, 1);
    load_m3(u, link_at(g, U, d, b), Gs);
    mm3(P, t, u);
    shift(d, g, b, 1);
    shift(d, g, a, -1);
    load_m3(u, link_at(g, U, d, a), Gs);
    mm3_nd(t, P, u);
    shift(d, g, a, -1);
    load_m3(u, link_at(g, U, d, a), Gs);
    mm3_nd(P, t, u);
    shift(d, g, b, -1);
    load_m3(u, link_at(g, U, d, b), Gs);
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < 9; e++) s += P[e].re * u[e].re + P[e].im * u[e].im;      // Re tr P u^+
    return s;
}
// a thread per site, all six planes, both orientations; wave sums by DPP, workgroup partial through LDS (every lane stays active: wave_sum needs all 64)
__global__ __launch_bounds__(256) void rect_sum_kernel(RectArgs k) {
    __shared__ double red[4];
    const int t = blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
    if (t < 2 * k.g.Vh) {
        const int p = t >= k.g.Vh ? 1 : 0, i = t - p * k.g.Vh;
        int c[4];
        cb_to_coords(k.g, p, i, c);
#pragma unroll 1
        for (int mu = 0; mu < 3; mu++)
#pragma unroll 1
            for (int nu = mu + 1; nu < 4; nu++) {
                acc += rect_retr(k.g, k.U, c, mu, nu);
                acc += rect_retr(k.g, k.U, c, nu, mu);
            }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) k.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

static int rect_supported(lqcd_ctx_s* c, const char* who) {
    if (!c->local_peers.empty()) {
        set_error(std::string(who) + ": not available on an in-process PE grid (a partitioned lattice: the rectangles need a halo of depth 2)");
        return LQCD_ERR_UNSUPPORTED;
    }
    if (any_partitioned(c)) {
        set_error(std::string(who) + ": the lattice is partitioned (the rectangles need a halo of depth 2)");
        return LQCD_ERR_UNSUPPORTED;
    }
    return LQCD_OK;
}

// sum over the 12 V rectangles of Re tr U_r, the workgroup partials added in the fixed order of reduce_to_slot: two calls give the same bits
static int rect_sum(lqcd_gauge_s* U, double* sum) {
    lqcd_ctx_s* c = U->ctx;
    HIPCHK(hipSetDevice(c->device));
    RectArgs k = {};
    k.g = c->geom;
    k.U = U->data;
    k.partial = c->d_partial;
    const int nb = (2 * c->geom.Vh + 255) / 256;
    hipLaunchKernelGGL(rect_sum_kernel, dim3(nb), dim3(256), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    LQCHK(reduce_to_slot(c, nb, 1, S_RED0, false, 0));
    HIPCHK(hipMemcpyAsync(c->h_scal, c->d_scal + S_RED0, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *sum = c->h_scal[0];
    return LQCD_OK;
}

// the staple sweep: mode 0 / 1 / 2 as the kernel's MODE
static int rect_sweep(lqcd_gauge_s* out, lqcd_gauge_s* U, double wp, double wr, double coef, double factor, int mode, int mu_only, int mu_out) {
    lqcd_ctx_s* c = U->ctx;
    HIPCHK(hipSetDevice(c->device));
    out->version++;     // arguments are valid: the field is about to be written
    RectArgs k = {};
    k.g = c->geom;
    k.U = U->data;
    k.out = out->data;
    k.wp = wp; k.wr = wr; k.coef = coef; k.factor = factor;
    k.mu_only = mu_only; k.mu_out = mu_out;
    k.bm = make_block_map(c->geom, c->tun.md_remap ? c->tun.xcd_remap : 0, c->tun.xcd_nsub, c->tun.xcd_ysplit);
    // links known to be on the group (tracked per version): two rows are loaded, the third rebuilt
    const bool r2 = c->tun.staple_recon && U->unitary_version == U->version;
    const dim3 grid(2 * c->geom.nch);
    if (mode == 0) { if (r2) hipLaunchKernelGGL((rect_force_kernel<0, true>), grid, dim3(256), 0, c->stream, k);
                     else hipLaunchKernelGGL((rect_force_kernel<0, false>), grid, dim3(256), 0, c->stream, k); }
    else if (mode == 1) { if (r2) hipLaunchKernelGGL((rect_force_kernel<1, true>), grid, dim3(256), 0, c->stream, k);
                          else hipLaunchKernelGGL((rect_force_kernel<1, false>), grid, dim3(256), 0, c->stream, k); }
    else { if (r2) hipLaunchKernelGGL((rect_force_kernel<2, true>), grid, dim3(64), 0, c->stream, k);
           else hipLaunchKernelGGL((rect_force_kernel<2, false>), grid, dim3(64), 0, c->stream, k); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

// mean of Re tr U_r / 3 over the 12 V rectangles: 1 on a cold field, normalised like lqcd_gauge_plaquette
extern "C" int lqcd_gauge_rectangle(lqcd_gauge_t U, double* rect) {
    LQCHK(links_flush_of(U));      // recorded single-direction link operations run first (links.hip)
    ARGCHK(U && rect, "lqcd_gauge_rectangle: null argument");
    lqcd_ctx_s* c = U->ctx;
    LQCHK(rect_supported(c, "lqcd_gauge_rectangle"));
    double sum = 0.0;
    LQCHK(rect_sum(U, &sum));
    const double V = (double)c->gL[0] * c->gL[1] * c->gL[2] * c->gL[3];
    *rect = sum / (12.0 * V * 3.0);
    return LQCD_OK;
}

// S_g = -(1/3) [ beta_plaq sum_plaq Re tr U_p + beta_rect sum_rect Re tr U_r ] = -V (6 beta_plaq plaquette + 12 beta_rect rectangle)
extern "C" int lqcd_gauge_action_improved(lqcd_gauge_t U, double beta_plaq, double beta_rect, double* Sg) {
    LQCHK(links_flush_of(U));
    ARGCHK(U && Sg, "lqcd_gauge_action_improved: null argument");
    lqcd_ctx_s* c = U->ctx;
    LQCHK(rect_supported(c, "lqcd_gauge_action_improved"));
    if (beta_rect == 0.0) return lqcd_gauge_action(U, beta_plaq, Sg);      // the plaquette action: today's path, bit for bit
    double plaq = 0.0, sum = 0.0;
    LQCHK(lqcd_gauge_plaquette(U, &plaq));
    LQCHK(rect_sum(U, &sum));
    const double V = (double)c->gL[0] * c->gL[1] * c->gL[2] * c->gL[3];
    *Sg = -beta_plaq * 6.0 * V * plaq - beta_rect * sum / 3.0;
    return LQCD_OK;
}

// G_mu(n) = -(1/6) U_mu(n) [ beta_plaq (plaquette staples) + beta_rect (rectangle staples) ]
extern "C" int lqcd_gauge_force_improved(lqcd_gauge_t out, lqcd_gauge_t U, double beta_plaq, double beta_rect) {
    LQCHK(links_flush_of(out));
    LQCHK(same_ctx(out, U, "lqcd_gauge_force_improved"));
    LQCHK(rect_supported(U->ctx, "lqcd_gauge_force_improved"));
    if (beta_rect == 0.0) return lqcd_gauge_force(out, U, beta_plaq);
    return rect_sweep(out, U, beta_plaq, beta_rect, -1.0 / 6.0, 0.0, 0, -1, 0);
}

// P_update! for this action in one pass: P += factor TA(G), the force field is never stored (P: traceless anti-Hermitian, lqcd_momentum_add_gauge_force)
extern "C" int lqcd_momentum_add_gauge_force_improved(lqcd_gauge_t P, double factor, lqcd_gauge_t U, double beta_plaq, double beta_rect) {
    LQCHK(links_flush_of(P));
    LQCHK(same_ctx(P, U, "lqcd_momentum_add_gauge_force_improved"));
    LQCHK(rect_supported(U->ctx, "lqcd_momentum_add_gauge_force_improved"));
    if (beta_rect == 0.0) return lqcd_momentum_add_gauge_force(P, factor, U, beta_plaq);
    return rect_sweep(P, U, beta_plaq, beta_rect, -1.0 / 6.0, factor, 1, -1, 0);
}

// calc_dSdUmu!(dSdUmu, gauge_action, mu, U) for this action: out[mu_out] = (beta_plaq/2) (plaquette staples) + (beta_rect/2) (rectangle staples) of direction mu --
// the normalisation of lqcd_link_staple.  Eager: not recorded, the mul! / Traceless_antihermitian_add! that follow run as the generic operations they are.
extern "C" int lqcd_link_staple_improved(lqcd_gauge_t out, int mu_out, lqcd_gauge_t U, int mu, double beta_plaq, double beta_rect) {
    LQCHK(links_flush_of(out));
    if (!(out && U && out->ctx == U->ctx && out != U && mu_out >= 0 && mu_out < 4 && mu >= 0 && mu < 4)) {
        set_error("lqcd_link_staple_improved: need two distinct gauge-shaped fields of one context and direction slots in 0..3");
        return LQCD_ERR_ARG;
    }
    LQCHK(rect_supported(U->ctx, "lqcd_link_staple_improved"));
    if (beta_rect == 0.0) return lqcd_link_staple(out, mu_out, U, mu, beta_plaq);
    return rect_sweep(out, U, 0.5 * beta_plaq, 0.5 * beta_rect, 0.0, 0.0, 2, mu, mu_out);
}
