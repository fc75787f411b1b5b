// staple.hip -- the staple sweep of the gauge side: the plaquette force G_mu(n) = -(beta/6) U_mu(n) (sum of the six staples) and everything fused onto it (the
// momentum update P += factor TA(G), the link update behind it, the RK3 stage of the gradient flow), its halo exchange on a partitioned lattice, and the
// drivers the other units call (staple_force, staple_force_expu, flow_stage, staple_halo_args; declared in gauge_staple.h).  Reference callers: P_update! /
// U_update! of src/md/AbstractMD.jl:78-118 (calc_dSdUmu!, Traceless_antihermitian_add!, exptU!); conventions: md.hip header.
//
// What this file ships is the only path.  Tried on one MI355X at 32^3x64 (ms per Sexton-Weingarten block U_update! P_update! U_update!, profiles/r06_staple_ab.log),
// lost, and removed -- each was a compile-time switch of md.hip, and its code is in the history before the gauge side was split into units:
//   right operands of the staple products loaded with all three rows (three row-2 rebuilds less per plane, 39 loads instead of 30)     1.416 -> 1.494
//   tile: the y rows from LDS too, through generic pointers (flat loads; 256 VGPRs, 19..51 spilled)                                      1.329 -> 1.483
//   tile: all three rows of a link in LDS (72 KiB, two workgroups per CU, no row-2 rebuild for operands from LDS)                       -1.7 % where rows 0, 1 give -5 %
//   tile: the five neighbour links of a plane in one load burst (214 VGPRs, two workgroups per CU)                                       1.332 against 1.317: no gain
// The switches whose other setting had lost earlier went with them: full three-row products in the two-row sweep, that sweep's loads in two groups instead of one
// burst, momenta and new links through the caches instead of past them (1.416 against 1.359), the tile with its own parity only, exp without Cayley-Hamilton.
#include "lqcd_internal.h"
#include "gauge_staple.h"

#include <algorithm>
#include <vector>

namespace lqcd {

// the one-sweep form streams the momenta (read + written once) and the new links (written once) past the caches: the block U_update! P_update! U_update!
// 1.416 -> 1.359 ms at 32^3x64 (profiles/r06_staple_ab.log) -- the sweep is bound by the memory path, not by issue
typedef double v2d_md __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cd ld_stream(const double2* p) {
    const v2d_md v = __builtin_nontemporal_load(reinterpret_cast<const v2d_md*>(p));
    return mk(v.x, v.y);
}
__device__ __forceinline__ void st_stream(double2* p, cd v) {
    const v2d_md t = {v.re, v.im};
    __builtin_nontemporal_store(t, reinterpret_cast<v2d_md*>(p));
}

// The partitioned-lattice instance: direction and plane stay run-time values here -- with the ghost-link and received-staple branches the
// fully templated body below needs > 256 registers (1000+ spilled); this form holds them in 256 without scratch.
template <int MODE>
__global__ __launch_bounds__(256) void gauge_force_kernel_part(GFArgs k) {
    constexpr bool FUSE_TA = MODE == 1 || MODE == 3 || MODE == 4;      // MODE 4: the RK3 stage of the gradient flow, X <- xscale X + factor TA(G)
    const Geom& g = k.g;
    const int p = blockIdx.x & 1, i = (blockIdx.x >> 1) * 64 + (threadIdx.x & 63), mu = (MODE == 2 || MODE == 3) ? k.mu_only : (int)(threadIdx.x >> 6);
    if (i >= g.Vh) return;
    const int Gs = glink_stride(g);
    int c[4];
    cb_to_coords(g, p, i, c);
    cd A[9];
#pragma unroll
    for (int e = 0; e < 9; e++) A[e] = mk(0.0, 0.0);
    for (int nu = 0; nu < 4; nu++) {
        if (nu == mu) continue;
        cd u1[9], u2[9], u3[9], t1[9], t2[9];
        link_fwd(u1, k, c, mu, nu);                         // U_nu(n+mu)
        link_fwd(u2, k, c, nu, mu);                         // U_mu(n+nu)
        load_m3(u3, link_at(g, k.U, c, nu), Gs);
        mm3_nd(t1, u1, u2);
        mm3_nd(t2, t1, u3);
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = A[e] + t2[e];
        if (c[nu] == 0 && g.part[nu]) {                     // n - nu lives on the -nu neighbour: its W arrived with the exchange
            const int Fh = face_half_sites(g, nu), f = coords_to_face(g, nu, c);
            const double2* b = k.wrecv[nu] + ((size_t)((1 - p) * 4 + mu) * 9) * Fh + f;
#pragma unroll
            for (int e = 0; e < 9; e++) t2[e] = ld(b + (size_t)e * Fh);
        } else {
            int m[4] = {c[0], c[1], c[2], c[3]};
            shift(m, g, nu, -1);
            lower_staple_at(t2, k, m, mu, nu);
        }
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = A[e] + t2[e];
    }
    const double coef = k.coef;
    if constexpr (MODE == 2) {
        double2* o2 = k.out + glink_off(g, p, k.mu_out, i);
#pragma unroll
        for (int e = 0; e < 9; e++) st(o2 + (size_t)e * Gs, mk(coef * A[e].re, coef * A[e].im));
        return;
    }
    cd um[9], r[9];
    load_m3(um, k.U + glink_off(g, p, mu, i), Gs);
    mm3(r, um, A);
    double2* o = k.out + glink_off(g, p, MODE == 3 ? k.mu_out : mu, i);
    if constexpr (!FUSE_TA) {
#pragma unroll
        for (int e = 0; e < 9; e++) st(o + (size_t)e * Gs, mk(coef * r[e].re, coef * r[e].im));
    } else {
        cd a[9];
        const double f = 0.5 * coef * k.factor;
#pragma unroll
        for (int x = 0; x < 3; x++)
#pragma unroll
            for (int y = 0; y < 3; y++) a[x * 3 + y] = mk(f * (r[x * 3 + y].re - r[y * 3 + x].re), f * (r[x * 3 + y].im + r[y * 3 + x].im));
        const double tr = (a[0].im + a[4].im + a[8].im) / 3.0;
        a[0].im -= tr; a[4].im -= tr; a[8].im -= tr;
        if constexpr (MODE == 4) {
            if (k.xread) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    const cd pv = ld(o + (size_t)e * Gs);
                    a[e] = mk(fma(k.xscale, pv.re, a[e].re), fma(k.xscale, pv.im, a[e].im));
                }
            }
#pragma unroll
            for (int e = 0; e < 9; e++) st(o + (size_t)e * Gs, a[e]);
            return;
        }
#pragma unroll
        for (int e = 0; e < 9; e++) {
            const cd pv = ld(o + (size_t)e * Gs);
            st(o + (size_t)e * Gs, mk(pv.re + a[e].re, pv.im + a[e].im));
        }
    }
}

// one plane (MU, NU) of the staple sum of link (n, MU): upper staple U_nu(n+mu) U_mu(n+nu)^+ U_nu(n)^+ and lower staple W_{mu nu}(n - nu).
// MU and NU are compile-time: every index into the by-value argument struct and the coordinate arrays is static.
__device__ __forceinline__ const double2* link_at_shifted(const Geom& g, const double2* __restrict__ U, const int (&c)[4], int dir, int step, int mu) {
    int d[4] = {c[0], c[1], c[2], c[3]};
    shift(d, g, dir, step);
    return link_at(g, U, d, mu);
}

template <int MODE, int MU, int NU, bool PART, bool R2>
__device__ __forceinline__ void staple_plane(cd (&A)[9], const GFArgs& k, int (&c)[4], int p, int lane, const double2 (*own)[9][64]) {
    if constexpr (MU != NU && R2 && !PART && MODE < 2) {
        // single GPU, links on the group: the five neighbour links of the plane are issued as ONE burst of two-row loads (30 x 1 KiB per wave: one
        // memory round trip per plane instead of two), row 2 is rebuilt as each link is consumed
        const Geom& g = k.g;
        const int Gs = glink_stride(g);
        cd a1[9], a2[9], l1[9], l2[9], l3[9], u3[9], t1[9], t2[9];
        int m[4] = {c[0], c[1], c[2], c[3]};
        shift(m, g, NU, -1);
        load_u_raw(a1, link_at_shifted(g, k.U, c, MU, 1, NU), Gs);      // U_nu(n+mu)
        load_u_raw(a2, link_at_shifted(g, k.U, c, NU, 1, MU), Gs);      // U_mu(n+nu)
        load_u_raw(l1, link_at_shifted(g, k.U, m, MU, 1, NU), Gs);      // U_nu(m+mu)
        load_u_raw(l2, link_at(g, k.U, m, MU), Gs);                     // U_mu(m)
        load_u_raw(l3, link_at(g, k.U, m, NU), Gs);                     // U_nu(m)
#pragma unroll
        for (int e = 0; e < 9; e++) { const double2 t = own[NU][e][lane]; u3[e] = mk(t.x, t.y); }
        // every staple is a product of SU(3) matrices: rows 0, 1 of each product (two thirds of the multiplications), row 2 rebuilt like a link's
        finish_u(a2);
        mm2_nd(t1, a1, a2);         // rows 0, 1 of a1 a2^+ need rows 0, 1 of a1 only
        mm2_nd(t2, t1, u3);
        finish_u(t2);
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = A[e] + t2[e];
        finish_u(l1);
        mm2(t1, l2, l1);            // Q = l2 l1, rows 0, 1
        finish_u(t1);
        finish_u(l3);
        mm2_dn(t2, t1, l3);         // rows 0, 1 of Q^+ l3 = l1^+ l2^+ l3
        finish_u(t2);
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = A[e] + t2[e];
        asm volatile("" : "+v"(c[0]), "+v"(A[0].re), "+v"(A[0].im), "+v"(A[4].re), "+v"(A[4].im), "+v"(A[8].re), "+v"(A[8].im));
    } else
    if constexpr (MU != NU) {
        const Geom& g = k.g;
        const int Gs = glink_stride(g);
        cd u1[9], u2[9], u3[9], t1[9], t2[9];
        link_fwd<PART, R2>(u1, k, c, MU, NU);               // U_nu(n+mu)
        link_fwd<PART, R2>(u2, k, c, NU, MU);               // U_mu(n+nu)
        if constexpr (MODE < 2) {
#pragma unroll
            for (int e = 0; e < 9; e++) { const double2 t = own[NU][e][lane]; u3[e] = mk(t.x, t.y); }
        } else {
            load_u<R2>(u3, link_at(g, k.U, c, NU), Gs);
        }
        mm3_nd(t1, u1, u2);
        mm3_nd(t2, t1, u3);
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = A[e] + t2[e];
        if (PART && c[NU] == 0 && g.part[NU]) {             // n - nu lives on the -nu neighbour: its W arrived with the exchange
            const int Fh = face_half_sites(g, NU), f = coords_to_face(g, NU, c);
            const double2* b = k.wrecv[NU] + ((size_t)((1 - p) * 4 + MU) * 9) * Fh + f;
#pragma unroll
            for (int e = 0; e < 9; e++) t2[e] = ld(b + (size_t)e * Fh);
        } else {
            int m[4] = {c[0], c[1], c[2], c[3]};
            shift(m, g, NU, -1);
            lower_staple_at<PART, R2>(t2, k, m, MU, NU);
        }
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = A[e] + t2[e];
        // the next plane's five link loads wait for this plane's sum: without the tie the scheduler hoists all fifteen of a direction (and
        // spills hundreds of registers); one plane in flight per wave, the other waves of the CU cover its latency
        asm volatile("" : "+v"(c[0]), "+v"(A[0].re), "+v"(A[0].im), "+v"(A[4].re), "+v"(A[4].im), "+v"(A[8].re), "+v"(A[8].im));
    }
}

// ---- TILE form of the staple plane (round 6): the workgroup keeps rows 0, 1 of the links of BOTH parities of its chunk in LDS -- a chunk of 64 checkerboard sites is
// 64 / XH whole x-rows, so with the other parity it is a closed (x, y) tile of 128 sites -- and the neighbour links at n + x / n - x (12 of the 60 loads per site) are
// read from there; the loads of a plane come in two groups (upper staple, then lower staple), which holds the kernel at 146..151 VGPRs: THREE workgroups per CU
// instead of two.  One Sexton-Weingarten block at 32^3x64: 1.339 -> 1.272 ms (profiles/r06_staple_ab.log).  The y rows of the tile (another 10.5 loads) would need a
// per-lane choice between LDS and global memory: generic pointers / flat loads, 256 registers and spills -- measured 12 % SLOWER (file header).
constexpr int STAPLE_TILE_ROWS = 6;     // components of a link in the tile's LDS copy: rows 0, 1 -- 2 parities x 4 directions x 6 x 64 double2 = 48 KiB per workgroup
constexpr int STAPLE_TILE_OCC = 3;      // ... so that three workgroups share a CU (at 146..151 VGPRs)
// lane of n + x / n - x inside the chunk of the other parity (x = 2 xh + q wraps inside its row)
__device__ __forceinline__ int tile_lane_px(int lane, int xh, int q, int XH) { return q ? (xh + 1 == XH ? lane - (XH - 1) : lane + 1) : lane; }
__device__ __forceinline__ int tile_lane_mx(int lane, int xh, int q, int XH) { return q ? lane : (xh == 0 ? lane + XH - 1 : lane - 1); }
template <int MU, int NU>
__device__ __forceinline__ void staple_plane_tile(cd (&A)[9], const GFArgs& k, int (&c)[4], int lane, const double2 (*own2)[4][STAPLE_TILE_ROWS][64]) {
    if constexpr (MU != NU) {
        const Geom& g = k.g;
        const int Gs = glink_stride(g), XH = g.XH;      // (the LDS copy has the component stride of the field: 64 elements)
        const int yr = lane / XH, xh = lane - yr * XH, q = c[0] & 1;
        // where the five neighbour links of the plane live: an x hop (MU == 0 / NU == 0) stays in the tile for every lane -- the other parity's copy, own2[1], a
        // ds_read; everything else is a global load.  Every select is made at compile time: never a flat load
        const int l_px = tile_lane_px(lane, xh, q, XH) & 63, l_mx = tile_lane_mx(lane, xh, q, XH) & 63;      // n + x, n - x
        int m[4] = {c[0], c[1], c[2], c[3]};
        shift(m, g, NU, -1);
        const double2* pa1 = MU == 0 ? &own2[1][NU][0][l_px] : link_at_shifted(g, k.U, c, MU, 1, NU);      // U_nu(n+mu)
        const double2* pa2 = NU == 0 ? &own2[1][MU][0][l_px] : link_at_shifted(g, k.U, c, NU, 1, MU);      // U_mu(n+nu)
        const double2* pl1 = link_at_shifted(g, k.U, m, MU, 1, NU);                                         // U_nu(m+mu): this parity, one hop outside the row
        const double2* pl2 = NU == 0 ? &own2[1][MU][0][l_mx] : link_at(g, k.U, m, MU);                      // U_mu(m)
        const double2* pl3 = NU == 0 ? &own2[1][NU][0][l_mx] : link_at(g, k.U, m, NU);                      // U_nu(m)
        cd a1[9], a2[9], l1[9], l2[9], l3[9], u3[9], t1[9], t2[9];
        // the upper staple: its global loads first; what is in LDS (the x cases) is read where it is used (short latency, no registers held across the loads)
        if constexpr (MU != 0) load_u_raw(a1, pa1, Gs);
        if constexpr (NU != 0) load_u_raw(a2, pa2, Gs);
        if constexpr (MU == 0) load_u_raw(a1, pa1, Gs);
        if constexpr (NU == 0) load_u_raw(a2, pa2, Gs);
        finish_u(a2);
        mm2_nd(t1, a1, a2);         // rows 0, 1 of a1 a2^+ need rows 0, 1 of a1 only
#pragma unroll
        for (int e = 0; e < STAPLE_TILE_ROWS; e++) { const double2 t = own2[0][NU][e][lane]; u3[e] = mk(t.x, t.y); }
        finish_u(u3);
        mm2_nd(t2, t1, u3);
        finish_u(t2);
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = A[e] + t2[e];
        asm volatile("" : "+v"(A[0].re), "+v"(A[4].im), "+v"(A[8].re));      // the lower staple's loads behind the upper staple's sum: 256 registers hold one staple at a time
        load_u_raw(l1, pl1, Gs);
        if constexpr (NU != 0) { load_u_raw(l2, pl2, Gs); load_u_raw(l3, pl3, Gs); }
        finish_u(l1);
        if constexpr (NU == 0) load_u_raw(l2, pl2, Gs);
        mm2(t1, l2, l1);            // Q = l2 l1, rows 0, 1
        finish_u(t1);
        if constexpr (NU == 0) load_u_raw(l3, pl3, Gs);
        finish_u(l3);
        mm2_dn(t2, t1, l3);         // rows 0, 1 of Q^+ l3 = l1^+ l2^+ l3
        finish_u(t2);
#pragma unroll
        for (int e = 0; e < 9; e++) A[e] = A[e] + t2[e];
        asm volatile("" : "+v"(c[0]), "+v"(A[0].re), "+v"(A[0].im), "+v"(A[4].re), "+v"(A[4].im), "+v"(A[8].re), "+v"(A[8].im));
    }
}

template <int MODE, int MU, bool PART, bool R2, bool EXPU = false, bool TILE = false, bool FLOW = false>
__device__ __forceinline__ void staple_links(const GFArgs& k, int p, int i, int lane, const double2 (*own)[9][64], const double2 (*own2)[4][STAPLE_TILE_ROWS][64] = nullptr) {
    constexpr bool FUSE_TA = MODE == 1 || MODE == 3;
    const Geom& g = k.g;
    const int Gs = glink_stride(g);
    int c[4];
    cb_to_coords(g, p, i, c);
    cd A[9];
#pragma unroll
    for (int e = 0; e < 9; e++) A[e] = mk(0.0, 0.0);
    if constexpr (TILE) {
        staple_plane_tile<MU, 0>(A, k, c, lane, own2);
        staple_plane_tile<MU, 1>(A, k, c, lane, own2);
        staple_plane_tile<MU, 2>(A, k, c, lane, own2);
        staple_plane_tile<MU, 3>(A, k, c, lane, own2);
    } else {
        staple_plane<MODE, MU, 0, PART, R2>(A, k, c, p, lane, own);
        staple_plane<MODE, MU, 1, PART, R2>(A, k, c, p, lane, own);
        staple_plane<MODE, MU, 2, PART, R2>(A, k, c, p, lane, own);
        staple_plane<MODE, MU, 3, PART, R2>(A, k, c, p, lane, own);
    }
    const double coef = k.coef;
    if constexpr (MODE == 2) {
        double2* o2 = k.out + glink_off(g, p, k.mu_out, i);
#pragma unroll
        for (int e = 0; e < 9; e++) st(o2 + (size_t)e * Gs, mk(coef * A[e].re, coef * A[e].im));
        return;
    }
    cd um[9], r[9];
    if constexpr (MODE == 3) load_m3(um, k.U + glink_off(g, p, MU, i), Gs);      // one direction per launch: the link comes from memory
    else if constexpr (TILE) {
#pragma unroll
        for (int e = 0; e < STAPLE_TILE_ROWS; e++) { const double2 t = own2[0][MU][e][lane]; um[e] = mk(t.x, t.y); }
        finish_u(um);
    } else {
#pragma unroll
        for (int e = 0; e < 9; e++) { const double2 t = own[MU][e][lane]; um[e] = mk(t.x, t.y); }      // U_mu(n) from LDS
    }
    mm3(r, um, A);
    double2* o = k.out + glink_off(g, p, MODE == 3 ? k.mu_out : MU, i);
    if constexpr (!FUSE_TA) {
#pragma unroll
        for (int e = 0; e < 9; e++) st(o + (size_t)e * Gs, mk(coef * r[e].re, coef * r[e].im));
    } else {
        cd a[9];
        const double f = 0.5 * coef * k.factor;
#pragma unroll
        for (int x = 0; x < 3; x++)
#pragma unroll
            for (int y = 0; y < 3; y++) a[x * 3 + y] = mk(f * (r[x * 3 + y].re - r[y * 3 + x].re), f * (r[x * 3 + y].im + r[y * 3 + x].im));
        const double tr = (a[0].im + a[4].im + a[8].im) / 3.0;
        a[0].im -= tr; a[4].im -= tr; a[8].im -= tr;
        // the momenta are anti-Hermitian (every writer of a momentum field stores TA matrices: the reference's p[mu] is a TA field by type), and so is the increment: the upper
        // triangle is read, the lower one follows -- bit for bit what the nine sums gave -- and 48 of the 144 bytes per link stay unread (profiles/r06_pmc_staple.log)
        auto addp = [&](auto E) {
            constexpr int e = decltype(E)::value;
            if constexpr (FLOW) {      // gradient-flow stage: X <- xscale X + factor TA(G); stage 1 (xread = 0) does not read X
                if (k.xread) {
                    const cd pv = ld_stream(o + (size_t)e * Gs);
                    a[e] = mk(fma(k.xscale, pv.re, a[e].re), fma(k.xscale, pv.im, a[e].im));
                }
            } else {
                const cd pv = EXPU ? ld_stream(o + (size_t)e * Gs) : ld(o + (size_t)e * Gs);
                a[e] = mk(pv.re + a[e].re, pv.im + a[e].im);
            }
        };
        addp(std::integral_constant<int, 0>()); addp(std::integral_constant<int, 1>()); addp(std::integral_constant<int, 2>());
        addp(std::integral_constant<int, 4>()); addp(std::integral_constant<int, 5>()); addp(std::integral_constant<int, 8>());
        a[3] = mk(-a[1].re, a[1].im); a[6] = mk(-a[2].re, a[2].im); a[7] = mk(-a[5].re, a[5].im);
#pragma unroll
        for (int e = 0; e < 9; e++) {
            if constexpr (EXPU) st_stream(o + (size_t)e * Gs, a[e]); else st(o + (size_t)e * Gs, a[e]);
        }
        if constexpr (EXPU) {      // the link update that follows this momentum update: exp(dt P_new) U_mu(n) into the second link buffer
            cd ex[9], t[9];
            exp_m3(ex, a, k.dt);
            mm3(t, ex, um);
            if (k.reunit) project_if_on_group(t, k.notproj);
            double2* uo = k.uout + glink_off(g, p, MU, i);
#pragma unroll
            for (int e = 0; e < 9; e++) st_stream(uo + (size_t)e * Gs, t[e]);
        }
    }
}

// out_mu(n) = coef * U_mu(n) * sum_{nu != mu} [ U_nu(n+mu) U_mu(n+nu)^+ U_nu(n)^+  +  W_{mu nu}(n - nu) ]
// workgroup = 64 sites of one parity x 4 waves (wave = mu, dispatched to a compile-time direction); the four links of the site go through
// LDS once (each wave loads its own direction: 36 KiB), the 6 x 2 neighbour links of a plane are re-used across waves/sites through L2.
// MODE 0: out = G.   MODE 1: out (the momenta) += factor * TA(G) -- P_update! in one pass, G never stored.
// MODE 2 (64-thread blocks, one direction): out[mu_out] = coef * (sum of the six staples of direction mu_only) -- the reference's
// calc_dSdUmu!(dSdUmu, gauge_action, mu, U) (AbstractMD.jl:108); the caller multiplies by U[mu] itself (mul!, :109).
// MODE 3 (64-thread blocks, one direction): out[mu_out] += factor * TA(coef U_mu * staples) -- the three calls of the reference's P_update! for one
// direction (calc_dSdUmu!, mul!, Traceless_antihermitian_add!: AbstractMD.jl:108-110) in one pass (lqcd_link_add_ta_staple).
constexpr int STAPLE_OCC = 2;      // workgroups per CU the register allocation is held to
template <int MODE, bool PART, bool R2 = false, bool EXPU = false, bool FLOW = false>
__global__ __launch_bounds__(256, STAPLE_OCC) void gauge_force_kernel(GFArgs k) {
    const Geom& g = k.g;
    int chunk, p;
    block_map(k.bm, blockIdx.x, chunk, p);
    const int lane = threadIdx.x & 63;
    const int i = chunk * 64 + lane;
    const int mu = MODE >= 2 ? k.mu_only : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool valid = i < g.Vh;
    __shared__ double2 own[MODE >= 2 ? 1 : 4][9][64];
    if constexpr (MODE < 2) {
        if (valid) {
            cd um[9];
            load_u<R2>(um, k.U + glink_off(g, p, mu, i), glink_stride(g));
#pragma unroll
            for (int e = 0; e < 9; e++) own[mu][e][lane] = mk2(um[e].re, um[e].im);
        }
        __syncthreads();
    }
    if (!valid) return;
    switch (mu) {
    case 0: staple_links<MODE, 0, PART, R2, EXPU, false, FLOW>(k, p, i, lane, own); break;
    case 1: staple_links<MODE, 1, PART, R2, EXPU, false, FLOW>(k, p, i, lane, own); break;
    case 2: staple_links<MODE, 2, PART, R2, EXPU, false, FLOW>(k, p, i, lane, own); break;
    default: staple_links<MODE, 3, PART, R2, EXPU, false, FLOW>(k, p, i, lane, own); break;
    }
}

// the TILE form (single GPU, links on the group, chunks of whole x-rows): MODE 0 / 1, optionally with the link update behind it.  LDS: rows 0, 1 of the links of both
// parities of the chunk: 48 KiB per workgroup, three workgroups per CU.
template <int MODE, bool EXPU, bool FLOW = false>
__global__ __launch_bounds__(256, STAPLE_TILE_OCC) void gauge_force_kernel_tile(GFArgs k) {
    const Geom& g = k.g;
    int chunk, p;
    block_map(k.bm, blockIdx.x, chunk, p);
    const int lane = threadIdx.x & 63;
    const int i = chunk * 64 + lane;
    const int mu = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ double2 own2[2][4][STAPLE_TILE_ROWS][64];      // [0]: this workgroup's parity, [1]: the other one
    {
        cd um[9], uo[9];
        load_u_raw(um, k.U + glink_off(g, p, mu, i), glink_stride(g));
        load_u_raw(uo, k.U + glink_off(g, 1 - p, mu, i), glink_stride(g));
#pragma unroll
        for (int e = 0; e < STAPLE_TILE_ROWS; e++) { own2[0][mu][e][lane] = mk2(um[e].re, um[e].im); own2[1][mu][e][lane] = mk2(uo[e].re, uo[e].im); }
    }
    __syncthreads();
    switch (mu) {
    case 0: staple_links<MODE, 0, false, true, EXPU, true, FLOW>(k, p, i, lane, nullptr, own2); break;
    case 1: staple_links<MODE, 1, false, true, EXPU, true, FLOW>(k, p, i, lane, nullptr, own2); break;
    case 2: staple_links<MODE, 2, false, true, EXPU, true, FLOW>(k, p, i, lane, nullptr, own2); break;
    default: staple_links<MODE, 3, false, true, EXPU, true, FLOW>(k, p, i, lane, nullptr, own2); break;
    }
}
// the tile form applies: a chunk is 64 / XH whole x-rows of one (z, t) plane (XH a divisor of 64, the rows of a plane divide into chunks, every chunk full)
static bool staple_tile_ok(lqcd_ctx_s* c) {
    const Geom& g = c->geom;
    return c->tun.staple_tile && g.XH >= 1 && g.XH <= 64 && 64 % g.XH == 0 && g.L[1] % (64 / g.XH) == 0 && g.Vh % 64 == 0 && !any_partitioned(c);
}

// upper nu-face of a partitioned direction nu = blockIdx.y: W_{mu nu}(m) for the three mu != nu, packed for the +nu neighbour
__global__ __launch_bounds__(128) void staple_face_kernel(GFArgs k) {
    const Geom& g = k.g;
    const int nu = blockIdx.y;
    if (!g.part[nu]) return;
    const int Fh = face_half_sites(g, nu);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * Fh) return;
    const int p = t / Fh, f = t - p * Fh;
    int m[4];
    face_to_coords(g, nu, g.L[nu] - 1, p, f, m);
    const int mc[4] = {m[0], m[1], m[2], m[3]};
    for (int mu = 0; mu < 4; mu++) {
        if (mu == nu) continue;
        cd w[9];
        lower_staple_at(w, k, mc, mu, nu);
        double2* b = k.wsend[nu] + ((size_t)(p * 4 + mu) * 9) * Fh + f;
#pragma unroll
        for (int e = 0; e < 9; e++) st(b + (size_t)e * Fh, w[e]);
    }
}

// ---- staple force on one rank / on a partitioned lattice
// Partitioned: (1) the x_lam = 0 link slices travel to the -lam neighbours (forward ghosts); (2) every rank computes the lower
// staples W_{mu nu} of its upper nu-faces (they need forward ghosts only) and sends them to the +nu neighbours; (3) the sweep
// reads ghosts for n+mu / n+nu and the received W for n-nu.  No corner exchange, two grouped send/recv steps.
static size_t gf_face_elems(lqcd_ctx_s* c, int mu) { return (size_t)2 * 4 * 9 * face_half_sites(c->geom, mu); }

static int gf_buffers(lqcd_ctx_s* c) {
    for (int mu = 0; mu < 4; mu++) {
        if (!c->geom.part[mu] || c->gf_ghost[mu]) continue;
        const size_t bytes = gf_face_elems(c, mu) * sizeof(double2);
        HIPCHK(hipMalloc((void**)&c->gf_ghost[mu], bytes));
        HIPCHK(hipMalloc((void**)&c->gf_gsend[mu], bytes));
        HIPCHK(hipMalloc((void**)&c->gf_wsend[mu], bytes));
        HIPCHK(hipMalloc((void**)&c->gf_wrecv[mu], bytes));
    }
    return LQCD_OK;
}

static GFArgs make_gfargs(lqcd_ctx_s* c, lqcd_gauge_s* U, lqcd_gauge_s* out, double beta, double factor) {
    GFArgs k;
    k.g = c->geom;
    k.U = U->data;
    k.out = out->data;
    k.coef = -beta / 6.0;
    k.factor = factor;
    k.mu_only = -1; k.mu_out = 0;
    k.uout = nullptr; k.dt = 0.0; k.notproj = nullptr; k.reunit = 0;
    k.xscale = 1.0; k.xread = 1;
    k.bm = make_block_map(c->geom, c->tun.md_remap ? c->tun.xcd_remap : 0, c->tun.xcd_nsub, c->tun.xcd_ysplit);
    for (int mu = 0; mu < 4; mu++) { k.ghost[mu] = c->gf_ghost[mu]; k.wrecv[mu] = c->gf_wrecv[mu]; k.wsend[mu] = c->gf_wsend[mu]; }
    return k;
}

static int launch_staple_faces(lqcd_ctx_s* c, const GFArgs& k) {
    int maxf = 0;
    for (int mu = 0; mu < 4; mu++)
        if (c->geom.part[mu]) maxf = std::max(maxf, face_half_sites(c->geom, mu));
    if (!maxf) return LQCD_OK;
    hipLaunchKernelGGL(staple_face_kernel, dim3((2 * maxf + 127) / 128, 4), dim3(128), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}
static int launch_staple_sweep(lqcd_ctx_s* c, const GFArgs& k, bool fuse, bool two_rows) {
    const dim3 grid(2 * c->geom.nch);
    // read-out for the tests (the same conditions as the dispatch below; a single-direction sweep has no tile form and loads two rows only where it is fused)
    c->tun.staple_form_active = any_partitioned(c) ? 3 : k.mu_only >= 0 ? (fuse && two_rows ? 1 : 0) : !two_rows ? 0 : staple_tile_ok(c) ? 2 : 1;
    if (any_partitioned(c)) {       // the instance with the ghost-link / received-staple branches
        if (k.mu_only >= 0 && fuse) hipLaunchKernelGGL(gauge_force_kernel_part<3>, grid, dim3(64), 0, c->stream, k);
        else if (k.mu_only >= 0) hipLaunchKernelGGL(gauge_force_kernel_part<2>, grid, dim3(64), 0, c->stream, k);
        else if (fuse) hipLaunchKernelGGL(gauge_force_kernel_part<1>, grid, dim3(256), 0, c->stream, k);
        else hipLaunchKernelGGL(gauge_force_kernel_part<0>, grid, dim3(256), 0, c->stream, k);
    } else {
        if (k.mu_only >= 0 && fuse) { if (two_rows) hipLaunchKernelGGL((gauge_force_kernel<3, false, true>), grid, dim3(64), 0, c->stream, k);
                                      else hipLaunchKernelGGL((gauge_force_kernel<3, false>), grid, dim3(64), 0, c->stream, k); }
        else if (k.mu_only >= 0) hipLaunchKernelGGL((gauge_force_kernel<2, false>), grid, dim3(64), 0, c->stream, k);
        else if (fuse) { if (two_rows && staple_tile_ok(c)) hipLaunchKernelGGL((gauge_force_kernel_tile<1, false>), grid, dim3(256), 0, c->stream, k);
                         else if (two_rows) hipLaunchKernelGGL((gauge_force_kernel<1, false, true>), grid, dim3(256), 0, c->stream, k);
                         else hipLaunchKernelGGL((gauge_force_kernel<1, false>), grid, dim3(256), 0, c->stream, k); }
        else { if (two_rows && staple_tile_ok(c)) hipLaunchKernelGGL((gauge_force_kernel_tile<0, false>), grid, dim3(256), 0, c->stream, k);
               else if (two_rows) hipLaunchKernelGGL((gauge_force_kernel<0, false, true>), grid, dim3(256), 0, c->stream, k);
               else hipLaunchKernelGGL((gauge_force_kernel<0, false>), grid, dim3(256), 0, c->stream, k); }
    }
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}

// send `sendb[mu]` to one neighbour and receive into `recvb[mu]` from the opposite one, all partitioned directions in one group
int gf_exchange_rccl(lqcd_ctx_s* c, double2* const sendb[4], double2* const recvb[4], bool to_backward) {
    ARGCHK(c->has_comm, "staple force: communicator not initialised (call lqcd_ctx_comm_init or lqcd_ctx_peer_init)");
    CommXfer x[4];
    int n = 0;
    for (int mu = 0; mu < 4; mu++) {
        if (!c->geom.part[mu]) continue;
        x[n++] = CommXfer{sendb[mu], recvb[mu], gf_face_elems(c, mu) * sizeof(double2), mu, to_backward ? 1 : 0};
    }
    return comm_sendrecv(c, x, n, c->stream, false);
}

// the two halo steps of a partitioned lattice, enqueued on the context's stream (nothing to do on one GPU).  Step 1, before the kernel arguments are made (it
// allocates the buffers they name): forward ghost links
int gauge_halo_links(lqcd_gauge_s* U) {
    lqcd_ctx_s* c = U->ctx;
    if (!any_partitioned(c)) return LQCD_OK;
    LQCHK(gf_buffers(c));
    for (int mu = 0; mu < 4; mu++)
        if (c->geom.part[mu]) LQCHK(gauge_pack_face(U, mu, c->gf_gsend[mu]));
    return gf_exchange_rccl(c, c->gf_gsend, c->gf_ghost, true);
}
// step 2: the lower staples of the upper faces to the +nu neighbours
static int staple_halo_lower(lqcd_ctx_s* c, const GFArgs& k) {
    if (!any_partitioned(c)) return LQCD_OK;
    LQCHK(launch_staple_faces(c, k));
    return gf_exchange_rccl(c, c->gf_wsend, c->gf_wrecv, false);
}
// the arguments of a staple kernel that reads the links of U as they are now (heatbath.hip), behind both halo steps
int staple_halo_args(lqcd_gauge_s* U, GFArgs& k) {
    lqcd_ctx_s* c = U->ctx;
    LQCHK(gauge_halo_links(U));
    k = make_gfargs(c, U, U, 0.0, 0.0);
    return staple_halo_lower(c, k);
}

int staple_force(lqcd_gauge_s* out, lqcd_gauge_s* U, double beta, double factor, bool fuse, int mu_only, int mu_out, double coef_override) {
    lqcd_ctx_s* c = U->ctx;
    HIPCHK(hipSetDevice(c->device));
    ARGCHK(!any_partitioned(c) || c->local_peers.empty(),
           "staple force: this context belongs to an in-process PE grid, use lqcd_mdom_gauge_force (fuse = 1 adds it to the momenta)");
    LQCHK(gauge_halo_links(U));
    out->version++;     // arguments are valid: the field is about to be written
    GFArgs k = make_gfargs(c, U, out, beta, factor);
    if (mu_only >= 0) { k.mu_only = mu_only; k.mu_out = mu_out; k.coef = coef_override; }
    LQCHK(staple_halo_lower(c, k));
    // links known to be on the group (tracked per version: generated there, measured, or projected by the link update): two rows are loaded
    LQCHK(launch_staple_sweep(c, k, fuse, c->tun.staple_recon && U->unitary_version == U->version));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LQCD_OK;
}

// the one-sweep forms (single GPU) write the new links to the context's spare link buffer -- the sweep reads the old links of the neighbours until its last
// workgroup -- and the two buffers change places in the handle
static int spare_links(lqcd_ctx_s* c, const lqcd_gauge_s* U) {
    if (c->gauge_spare) return LQCD_OK;
    HIPCHK(hipMalloc((void**)&c->gauge_spare, U->elems * sizeof(double2)));
    HIPCHK(hipMemsetAsync(c->gauge_spare, 0, U->elems * sizeof(double2), c->stream));      // stride padding stays zero
    return LQCD_OK;
}
template <bool FLOW>
static void launch_sweep_expu(lqcd_ctx_s* c, const GFArgs& k, bool two_rows) {
    const dim3 grid(2 * c->geom.nch);
    c->tun.staple_form_active = !two_rows ? 0 : staple_tile_ok(c) ? 2 : 1;
    if (two_rows && staple_tile_ok(c)) hipLaunchKernelGGL((gauge_force_kernel_tile<1, true, FLOW>), grid, dim3(256), 0, c->stream, k);
    else if (two_rows) hipLaunchKernelGGL((gauge_force_kernel<1, false, true, true, FLOW>), grid, dim3(256), 0, c->stream, k);
    else hipLaunchKernelGGL((gauge_force_kernel<1, false, false, true, FLOW>), grid, dim3(256), 0, c->stream, k);
}

// P_update! followed by U_update! (what every Sexton-Weingarten block of runMD_QPQ_sw! asks for, standardMD.jl:150-152) in ONE sweep over the links, single
// GPU: P += factor TA(-(beta/6) U staples), then U' = exp(dt P) U with the momentum still in registers.  Moves 576 (U) + 1152 (P r/w) + 576 (U')
// B/site where the two separate passes move 3456.
int staple_force_expu(lqcd_gauge_s* P, lqcd_gauge_s* U, double beta, double factor, double dt) {
    lqcd_ctx_s* c = U->ctx;
    HIPCHK(hipSetDevice(c->device));
    LQCHK(spare_links(c, U));
    GFArgs k = make_gfargs(c, U, P, beta, factor);
    k.uout = c->gauge_spare; k.dt = dt; k.reunit = c->tun.md_reunitarize;
    const bool two_rows = c->tun.staple_recon && U->unitary_version == U->version;
    P->version++;
    bool all_projected;
    LQCHK(launch_with_notproj_flag(c, k.reunit, &all_projected, [&](unsigned* flag) {
        k.notproj = flag;
        launch_sweep_expu<false>(c, k, two_rows);
    }));
    std::swap(U->data, c->gauge_spare);
    U->version++;
    if (all_projected) U->unitary_version = U->version;      // every link was projected: the field is on the group to rounding
    return LQCD_OK;
}

// One RK3 stage of the Wilson gradient flow (flow.hip): X <- xscale X + factor TA(G(U)) with G the staple force at beta = 6 (Z = TA(G), md.hip header), then
// U <- exp(X) U.  Single GPU: ONE sweep, the staple_force_expu form with the accumulator scaled before the add.  Partitioned: the halo steps of staple_force,
// the sweep into X, then the exponential update as a second pass (md.hip).  Nothing is synchronised with the host: *notproj (device word, cleared by the
// caller) is set when some link was not projected back onto the group (md_reunitarize).
int flow_stage(lqcd_gauge_s* U, double2* X, double xscale, double factor, bool xread, unsigned* notproj, bool two_rows) {
    lqcd_ctx_s* c = U->ctx;
    const int reunit = c->tun.md_reunitarize;
    if (!any_partitioned(c)) {
        LQCHK(spare_links(c, U));
        GFArgs k = make_gfargs(c, U, U, 6.0, factor);
        k.out = X;
        k.uout = c->gauge_spare; k.dt = 1.0; k.notproj = notproj; k.reunit = reunit;
        k.xscale = xscale; k.xread = xread ? 1 : 0;
        launch_sweep_expu<true>(c, k, two_rows);
        HIPCHK(hipGetLastError());
        std::swap(U->data, c->gauge_spare);      // stream order: the next launch reads the new links
        U->version++;
        return LQCD_OK;
    }
    ARGCHK(c->local_peers.empty(), "gradient flow: this context belongs to an in-process PE grid");
    LQCHK(gauge_halo_links(U));
    GFArgs k = make_gfargs(c, U, U, 6.0, factor);
    k.out = X;
    k.xscale = xscale; k.xread = xread ? 1 : 0;
    LQCHK(staple_halo_lower(c, k));
    c->tun.staple_form_active = 3;
    hipLaunchKernelGGL(gauge_force_kernel_part<4>, dim3(2 * c->geom.nch), dim3(256), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    LQCHK(link_exp_update_enqueue(U, 1.0, X, reunit != 0, notproj));
    U->version++;
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

// G_mu(n) = -(beta/6) U_mu(n) * (sum of the six staples)      (calc_dSdUmu! + mul!(temp, U, dSdUmu), AbstractMD.jl:108-110)
extern "C" int lqcd_gauge_force(lqcd_gauge_t out, lqcd_gauge_t U, double beta) {
    LQCHK(links_flush_of(out));      // recorded single-direction link operations run first (links.hip)
    LQCHK(same_ctx(out, U, "lqcd_gauge_force"));
    return staple_force(out, U, beta, 0.0, false);
}

// the same on an in-process PE grid (tests): arrays ordered by rank; fuse = 0 writes the force field, 1 accumulates into momenta
extern "C" int lqcd_mdom_gauge_force(int n, lqcd_gauge_t* outs, lqcd_gauge_t* Us, double beta, double factor, int fuse) {
    ARGCHK(outs && Us && n >= 1, "lqcd_mdom_gauge_force: null");
    lqcd_ctx_s* c0 = Us[0]->ctx;
    ARGCHK((int)c0->local_peers.size() == n, "lqcd_mdom_gauge_force: contexts are not linked with lqcd_ctx_link_local (or wrong n)");
    std::vector<GFArgs> ks(n);
    for (int r = 0; r < n; r++) {
        LQCHK(same_ctx(outs[r], Us[r], "lqcd_mdom_gauge_force"));
        lqcd_ctx_s* c = Us[r]->ctx;
        ARGCHK(c->rank == r, "lqcd_mdom_gauge_force: fields must be ordered by rank");
        HIPCHK(hipSetDevice(c->device));
        LQCHK(gf_buffers(c));
        outs[r]->version++;
    }
    for (int r = 0; r < n; r++) {          // forward ghosts: the x_mu = 0 slice of the +mu neighbour
        lqcd_ctx_s* c = Us[r]->ctx;
        for (int mu = 0; mu < 4; mu++)
            if (c->geom.part[mu]) LQCHK(gauge_pack_face(Us[c->nbr_fwd[mu]], mu, c->gf_ghost[mu]));
    }
    HIPCHK(hipDeviceSynchronize());
    for (int r = 0; r < n; r++) {
        ks[r] = make_gfargs(Us[r]->ctx, Us[r], outs[r], beta, factor);
        LQCHK(launch_staple_faces(Us[r]->ctx, ks[r]));
    }
    HIPCHK(hipDeviceSynchronize());
    for (int r = 0; r < n; r++) {          // lower staples of the upper nu-face -> the +nu neighbour
        lqcd_ctx_s* c = Us[r]->ctx;
        for (int mu = 0; mu < 4; mu++)
            if (c->geom.part[mu])
                HIPCHK(hipMemcpy(Us[c->nbr_fwd[mu]]->ctx->gf_wrecv[mu], c->gf_wsend[mu], gf_face_elems(c, mu) * sizeof(double2), hipMemcpyDeviceToDevice));
    }
    HIPCHK(hipDeviceSynchronize());
    for (int r = 0; r < n; r++) LQCHK(launch_staple_sweep(Us[r]->ctx, ks[r], fuse != 0, false));
    HIPCHK(hipDeviceSynchronize());
    return LQCD_OK;
}
