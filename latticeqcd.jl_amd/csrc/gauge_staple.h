// gauge_staple.h -- 3x3 link algebra and the staple helpers shared by the staple-force sweeps (md.hip) and the heatbath (heatbath.hip): link loads,
// products, the forward-ghost / lower-staple reads of a partitioned lattice, and the projection back onto SU(3).
#pragma once
#include "lqcd_internal.h"

namespace lqcd {

__device__ __forceinline__ void load_m3(cd (&u)[9], const double2* __restrict__ base, int stride) {
#pragma unroll
    for (int e = 0; e < 9; e++) u[e] = ld(base + (size_t)e * stride);
}
// C = A B
__device__ __forceinline__ void mm3(cd (&C)[9], const cd (&A)[9], const cd (&B)[9]) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            cd t = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) cfma(t, A[a * 3 + k], B[k * 3 + b]);
            C[a * 3 + b] = t;
        }
}
// C = A B^+
__device__ __forceinline__ void mm3_nd(cd (&C)[9], const cd (&A)[9], const cd (&B)[9]) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            cd t = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) cfma_conj(t, B[b * 3 + k], A[a * 3 + k]);
            C[a * 3 + b] = t;
        }
}
// C = A^+ B
__device__ __forceinline__ void mm3_dn(cd (&C)[9], const cd (&A)[9], const cd (&B)[9]) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            cd t = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) cfma_conj(t, A[k * 3 + a], B[k * 3 + b]);
            C[a * 3 + b] = t;
        }
}
// rows 0, 1 of C = A B / A B^+ / A^+ B (row 2 of C is left alone: a product of SU(3) matrices gets it from finish_u)
__device__ __forceinline__ void mm2(cd (&C)[9], const cd (&A)[9], const cd (&B)[9]) {
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            cd t = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) cfma(t, A[a * 3 + k], B[k * 3 + b]);
            C[a * 3 + b] = t;
        }
}
__device__ __forceinline__ void mm2_nd(cd (&C)[9], const cd (&A)[9], const cd (&B)[9]) {
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            cd t = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) cfma_conj(t, B[b * 3 + k], A[a * 3 + k]);
            C[a * 3 + b] = t;
        }
}
__device__ __forceinline__ void mm2_dn(cd (&C)[9], const cd (&A)[9], const cd (&B)[9]) {
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            cd t = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) cfma_conj(t, A[k * 3 + a], B[k * 3 + b]);
            C[a * 3 + b] = t;
        }
}
// C = A^+ B^+ = (B A)^+
__device__ __forceinline__ void mm3_dd(cd (&C)[9], const cd (&A)[9], const cd (&B)[9]) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            cd t = mk(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) cfma(t, B[b * 3 + k], A[k * 3 + a]);
            C[a * 3 + b] = mk(t.re, -t.im);
        }
}

// links of a field that is known to be on the group (lqcd_gauge_s::unitary_version): rows 0 and 1 from memory, row 2 = conj(row 0 x row 1) --
// two thirds of the bytes through the L1 / L2 path, which is what bounds the staple sweep (60 neighbour-link loads per site)
template <bool R2>
__device__ __forceinline__ void load_u(cd (&u)[9], const double2* __restrict__ base, int stride) {
    if constexpr (!R2) { load_m3(u, base, stride); return; }
#pragma unroll
    for (int e = 0; e < 6; e++) u[e] = ld(base + (size_t)e * stride);
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const int b1 = (b + 1) % 3, b2 = (b + 2) % 3;
        const cd x = cmul(u[b1], u[3 + b2]) - cmul(u[b2], u[3 + b1]);
        u[6 + b] = mk(x.re, -x.im);
    }
}

// link U_mu at the site with local coordinates c (periodic wrap; links carry no boundary sign)
__device__ __forceinline__ const double2* link_at(const Geom& g, const double2* __restrict__ U, const int (&c)[4], int mu) {
    const int p = (c[0] + c[1] + c[2] + c[3]) & 1;
    return U + glink_off(g, p, mu, coords_to_cb(g, c));
}
__device__ __forceinline__ void shift(int (&d)[4], const Geom& g, int mu, int dir) {
    d[mu] += dir;
    if (d[mu] == g.L[mu]) d[mu] = 0;
    if (d[mu] < 0) d[mu] = g.L[mu] - 1;
}

// arguments of the staple kernels.  Partitioned lattice: ghost[lam] = the x_lam = 0 slice of all links of the +lam neighbour
// ([parity][nu][9][Fh], fields.hip gauge_face_pack), wrecv[nu] = the lower staples W_{mu nu} of the -nu neighbour's upper face
// ([parity of that site][mu][9][Fh]); both null on a single GPU.
struct GFArgs {
    Geom g;
    const double2* U;
    double2* out;
    double coef, factor;
    const double2* ghost[4];
    const double2* wrecv[4];
    double2* wsend[4];
    BlockMap bm;             // workgroup -> chunk map of the sweep (tunable md_remap: 1 = the Dslash kernels' XCD tile sweep, 0 = plain order)
    int mu_only, mu_out;     // MODE 2 (calc_dSdUmu!): only direction mu_only, staple sum written to direction slot mu_out of `out`
    // EXPU instances (P_update! and the U_update! that follows it in ONE sweep): uout <- exp(dt P_new) U, a second link buffer (the sweep still reads the old links)
    double2* uout;
    double dt;
    unsigned* notproj;
    int reunit;
    // FLOW instances (one RK3 stage of the gradient flow, flow.hip): the accumulator X in `out` becomes xscale X + factor TA(G) -- xread = 0 (stage 1): X is not read
    double xscale;
    int xread;
};

// U_nu at the site c + dir_hat: local, or from the forward ghost slice when the step leaves the rank
template <bool PART = true, bool R2 = false>
__device__ __forceinline__ void link_fwd(cd (&u)[9], const GFArgs& k, const int (&c)[4], int dir, int nu) {
    const Geom& g = k.g;
    int d[4] = {c[0], c[1], c[2], c[3]};
    d[dir] += 1;
    if (d[dir] == g.L[dir]) {
        d[dir] = 0;
        if (PART && g.part[dir]) {
            const int p = (d[0] + d[1] + d[2] + d[3]) & 1, Fh = face_half_sites(g, dir), f = coords_to_face(g, dir, d);
            const double2* b = k.ghost[dir] + ((size_t)(p * 4 + nu) * 9) * Fh + f;
#pragma unroll
            for (int e = 0; e < 9; e++) u[e] = ld(b + (size_t)e * Fh);
            return;
        }
    }
    load_u<R2>(u, link_at(g, k.U, d, nu), glink_stride(g));
}

// lower staple seen from the site m = n - nu_hat:  W_{mu nu}(m) = U_nu(m+mu)^+ U_mu(m)^+ U_nu(m)
template <bool PART = true, bool R2 = false>
__device__ __forceinline__ void lower_staple_at(cd (&w)[9], const GFArgs& k, const int (&m)[4], int mu, int nu) {
    cd u1[9], u2[9], u3[9], t1[9];
    const int Gs = glink_stride(k.g);
    link_fwd<PART, R2>(u1, k, m, mu, nu);
    load_u<R2>(u2, link_at(k.g, k.U, m, mu), Gs);
    load_u<R2>(u3, link_at(k.g, k.U, m, nu), Gs);
    mm3_dd(t1, u1, u2);
    mm3(w, t1, u3);
}

// Back onto SU(3): rows 0 and 1 by Gram-Schmidt, row 2 = conj(row 0 x row 1) with the arithmetic of the 12-real gate (fields.hip
// gauge_compress12), so a projected link passes that gate with deviation 0.  For a link that is unitary up to accumulated rounding the
// change is of the order of that rounding.
__device__ __forceinline__ void reunitarize_m3(cd (&u)[9]) {
    double n0 = 0.0;
#pragma unroll
    for (int b = 0; b < 3; b++) n0 += u[b].re * u[b].re + u[b].im * u[b].im;
    const double i0 = 1.0 / sqrt(n0);
#pragma unroll
    for (int b = 0; b < 3; b++) u[b] = mk(i0 * u[b].re, i0 * u[b].im);
    cd d = mk(0.0, 0.0);      // <row0, row1>
#pragma unroll
    for (int b = 0; b < 3; b++) cfma_conj(d, u[b], u[3 + b]);
    double n1 = 0.0;
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const cd pr = cmul(d, u[b]);
        u[3 + b] = mk(u[3 + b].re - pr.re, u[3 + b].im - pr.im);
        n1 += u[3 + b].re * u[3 + b].re + u[3 + b].im * u[3 + b].im;
    }
    const double i1 = 1.0 / sqrt(n1);
#pragma unroll
    for (int b = 0; b < 3; b++) u[3 + b] = mk(i1 * u[3 + b].re, i1 * u[3 + b].im);
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const int b1 = (b + 1) % 3, b2 = (b + 2) % 3;
        const cd x = cmul(u[b1], u[3 + b2]) - cmul(u[b2], u[3 + b1]);
        u[6 + b] = mk(x.re, -x.im);
    }
}

}  // namespace lqcd
