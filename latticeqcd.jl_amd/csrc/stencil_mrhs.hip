// stencil_mrhs.hip -- the direction-split Wilson parity hop on several right-hand sides ("columns") that share the gauge field:
//     out_j = a xin_j + b H in_j ,   j < n                     (Wilson r = 1, fp64, one unpartitioned GPU, Vh a multiple of 64)
// The workgroup shape of the single-column kernel (stencil.hip wilson_dirsplit): 4 waves own 64 consecutive checkerboard sites, wave w does direction w.  The wave
// loads the two links of its direction ONCE and keeps them in registers, then walks the columns: neighbour half-spinors, two colour mat-vecs, reconstruct, the four
// direction partials through the part[4][12][64] LDS tile (one 48 KiB tile re-used by every column, two barriers per column), wave w stores spin row w.  Per output
// site the links cost 768 B / NB instead of 768 B (12-real links).  Every column runs the arithmetic of the single-column kernel (the helpers of stencil_common.h, the
// (s0 + s1) + (s2 + s3) combine), whatever its slot: columns are independent bit for bit.
// DOT: per column and workgroup Re / Im <z_j, out_j> and |out_j|^2 with the fixed-order wave and workgroup sums of the single-column dot epilogue.
// A column whose done word is non-zero is skipped by a workgroup-uniform branch (no loads, no stores, no barriers); the word is read from memory that no kernel of
// the same launch writes (the solver's scalar steps are launches of their own), so every wave of every workgroup takes the same branch.
// Plain launches: no grid-wide synchronisation, no spin waits, no persistent workgroups.
#include "stencil_common.h"
#include "ops_internal.h"

namespace lqcd {
inline namespace LQCD_PNS {

constexpr int MR_NB = 4;      // columns per launch

// Registers: both links stay resident across the column loop, so the budget of three workgroups per CU (168 VGPRs) is tight.  The 12-real instances keep the
// two stored rows (48 VGPRs for both links) and rebuild row 2 per column and hop, the 18-real instances keep all 72; every instance compiles to 168 VGPRs
// without scratch (DESIGN.md section 16 lists what it took).

struct MCols {
    real2* out[2][MR_NB];
    const real2* in[2][MR_NB];
    const real2* xin[2][MR_NB];
    const real2* z[MR_NB];
    double* dot[MR_NB];
    const double* done[MR_NB];
    int conj;
};

// entry j of a small table held in kernel arguments, without a dynamic index (which would send the argument struct through scratch)
template <typename T>
__device__ __forceinline__ T pick4(T const (&t)[MR_NB], int j) {
    T p = t[0];
    p = j == 1 ? t[1] : p; p = j == 2 ? t[2] : p; p = j == 3 ? t[3] : p;
    return p;
}

// the two colour mat-vecs of one hop with the link in registers: the arithmetic of wilson_hop in front of its reconstruct
template <int MU, int S, bool ADJ, int NL>
__device__ __forceinline__ void mrhs_chi(cd (&chi0)[3], cd (&chi1)[3], const real2* __restrict__ psi, const cd (&ul)[NL], int Vh, real sign) {
    cd h0[3], h1[3], u[9];
    project<MU, S>(h0, h1, psi, Vh);
#pragma unroll
    for (int q = 0; q < NL; q++) u[q] = ul[q];
    if constexpr (NL == 6) recon_row2(u);
    if (__builtin_amdgcn_ballot_w64(sign != real(1.0)) != 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) { h0[c] = sign * h0[c]; h1[c] = sign * h1[c]; }
    }
    su3_mv<ADJ>(chi0, u, h0);
    su3_mv<ADJ>(chi1, u, h1);
}
// both hops of direction MU.  The forward hop's two rows wait (6 complex numbers) while the backward hop is computed and both are reconstructed at the end -- the
// additions of wilson_hop, forward first, so the same bits, with 24 VGPRs less across the second hop than the 12-component partial spinor
template <int MU, bool DAG, int NL>
__device__ __forceinline__ void mrhs_hops(cd (&acc)[12], const real2* __restrict__ psi, const cd (&uf)[NL], const cd (&ub)[NL], unsigned onf, unsigned onb, real sf, real sb, int Vh) {
    constexpr int SF = DAG ? -1 : 1;
    cd f0[3], f1[3], b0[3], b1[3];
    mrhs_chi<MU, SF, false, NL>(f0, f1, psi + onf, uf, Vh, sf);
    __builtin_amdgcn_sched_barrier(0);      // the backward hop's twelve loads are not hoisted over the forward hop's arithmetic: with both links resident there is no room for them
    mrhs_chi<MU, -SF, true, NL>(b0, b1, psi + onb, ub, Vh, sb);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 12; q++) acc[q] = mk(0.0, 0.0);
    reconstruct<MU, SF>(acc, f0, f1);
    reconstruct<MU, -SF>(acc, b0, b1);
}

// neighbour sites and boundary signs of direction MU (a Nbr of its own per direction: every index static)
template <int MU>
__device__ __forceinline__ void mrhs_nbr(const Geom& g, int p, int i, int& nf, int& nb, real& sf, real& sb) {
    Nbr n;
    int c[4];
    neighbours(g, p, i, n, c);
    nf = n.fwd[MU]; nb = n.bwd[MU]; sf = n.sf[MU]; sb = n.sb[MU];
}

template <bool DAG, bool R12, bool DOT, int NB>
__global__ __launch_bounds__(256, 3) void wilson_mrhs(KArgs k, MCols m) {
    __shared__ real2 part[4][12][64];  // 48 KiB, one tile for every column
    __shared__ double red[DOT ? 12 : 1];
    constexpr int NL = R12 ? 6 : 9;      // complex numbers kept per link
    int chunk, p;
    map_block(k, chunk, p);
    const int Vh = sp_stride(k.g);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int i = chunk * 64 + lane;      // (the launcher requires Vh % 64 == 0: every lane owns a site)
    int nf, nb;
    real sf_, sb_;
    switch (w) {
    case 0: mrhs_nbr<0>(k.g, p, i, nf, nb, sf_, sb_); break;
    case 1: mrhs_nbr<1>(k.g, p, i, nf, nb, sf_, sb_); break;
    case 2: mrhs_nbr<2>(k.g, p, i, nf, nb, sf_, sb_); break;
    default: mrhs_nbr<3>(k.g, p, i, nf, nb, sf_, sb_); break;
    }
    // the two links of this wave's direction, once for all columns
    cd uf[NL], ub[NL];
    {
        const real2* __restrict__ Uf = R12 ? k.gauge12 + gl12_off(k.g, p, w, i) : k.gauge + glink_off(k.g, p, w, i);
        const real2* __restrict__ Ub = R12 ? k.gauge12 + gl12_off(k.g, 1 - p, w, nb) : k.gauge + glink_off(k.g, 1 - p, w, nb);
        const int us = R12 ? 64 : glink_stride(k.g);
#pragma unroll
        for (int q = 0; q < NL; q++) { uf[q] = ld(Uf + (size_t)q * us); ub[q] = ld(Ub + (size_t)q * us); }
    }
    // what stays live across the column loop beside the links is kept narrow: 32-bit element offsets, the boundary signs (+-1: exact) as floats
    const unsigned own = (unsigned)sp12_off(i), onf = (unsigned)sp12_off(nf), onb = (unsigned)sp12_off(nb);
    const float sf = (float)sf_, sb = (float)sb_;
    __builtin_amdgcn_sched_barrier(0);      // (a column's loads are not hoisted in front of the links': there is no room for both)
    bool first = true;
    int ncol = NB;
    asm volatile("" : "+s"(ncol));      // NB is the trip count only: every instance keeps the loop (unrolled or dropped, a column's loads mix with the links' and spill)
#pragma unroll 1
    for (int j = 0; j < ncol; j++) {
        const double* dn = pick4(m.done, j);
        if (dn && *dn != 0.0) continue;      // (the same in every wave of every workgroup: the word is not written during this launch)
        if (!first) __syncthreads();         // the combine of the column before has read the tile
        first = false;
        const real2* __restrict__ psi = p ? pick4(m.in[0], j) : pick4(m.in[1], j);
        const real2* __restrict__ xin = p ? pick4(m.xin[1], j) : pick4(m.xin[0], j);
        real2* __restrict__ out = p ? pick4(m.out[1], j) : pick4(m.out[0], j);
        cd acc[12];
        switch (w) {
        case 0: mrhs_hops<0, DAG, NL>(acc, psi, uf, ub, onf, onb, (real)sf, (real)sb, Vh); break;
        case 1: mrhs_hops<1, DAG, NL>(acc, psi, uf, ub, onf, onb, (real)sf, (real)sb, Vh); break;
        case 2: mrhs_hops<2, DAG, NL>(acc, psi, uf, ub, onf, onb, (real)sf, (real)sb, Vh); break;
        default: mrhs_hops<3, DAG, NL>(acc, psi, uf, ub, onf, onb, (real)sf, (real)sb, Vh); break;
        }
        cd xv[3] = {mk(0, 0), mk(0, 0), mk(0, 0)};
        if (k.a != 0.0) {      // the diagonal term, requested behind the hops (no long live range); the LDS exchange and the barrier cover the load
#pragma unroll
            for (int cc = 0; cc < 3; cc++) xv[cc] = ld(xin + own + co12(3 * w + cc));
        }
        cd zv[DOT ? 3 : 1];
        if constexpr (DOT) {
            const real2* __restrict__ z = pick4(m.z, j);
#pragma unroll
            for (int cc = 0; cc < 3; cc++) zv[cc] = (z == xin && k.a != 0.0) ? xv[cc] : ld(z + own + co12(3 * w + cc));
        }
#pragma unroll
        for (int q = 0; q < 12; q++) part[w][q][lane] = mk2(acc[q].re, acc[q].im);
        __syncthreads();
        real nrm = 0.0, dre = 0.0, dim = 0.0;
#pragma unroll
        for (int cc = 0; cc < 3; cc++) {
            const int q = 3 * w + cc;
            const real2 s0 = part[0][q][lane], s1 = part[1][q][lane], s2 = part[2][q][lane], s3 = part[3][q][lane];
            const cd s = mk((s0.x + s1.x) + (s2.x + s3.x), (s0.y + s1.y) + (s2.y + s3.y));
            cd v = k.b * s;
            v = mk(fma(k.a, xv[cc].re, v.re), fma(k.a, xv[cc].im, v.im));
            if (k.nt & 4) st_nt(out + own + co12(q), v); else st(out + own + co12(q), v);
            if constexpr (DOT) {        // <z, v> = conj(z) v
                nrm = fma(v.re, v.re, nrm); nrm = fma(v.im, v.im, nrm);
                dre = fma(zv[cc].re, v.re, dre); dre = fma(zv[cc].im, v.im, dre);
                dim = fma(zv[cc].re, v.im, dim); dim = fma(-zv[cc].im, v.re, dim);
            }
        }
        if constexpr (DOT) {            // three sums per column and workgroup: a wave tree each, then the four waves in a fixed order
            double t3[3] = {(double)dre, (double)(m.conj ? -dim : dim), (double)nrm};
#pragma unroll
            for (int q = 0; q < 3; q++) {
                t3[q] = wave_sum(t3[q]);
                if (lane == 0) red[4 * q + w] = t3[q];
            }
            __syncthreads();            // (also orders this column's tile reads before the next column's tile writes)
            first = true;
            double* dp = pick4(m.dot, j);
            if ((int)threadIdx.x < 3) dp[3 * (size_t)blockIdx.x + threadIdx.x] = (red[4 * threadIdx.x] + red[4 * threadIdx.x + 1]) + (red[4 * threadIdx.x + 2] + red[4 * threadIdx.x + 3]);
        }
    }
}

template <bool DAG, bool R12, bool DOT>
static void mrhs_launch_nb(int nb, dim3 grid, hipStream_t st, const KArgs& k, const MCols& m) {
    switch (nb) {
    case 1: hipLaunchKernelGGL((wilson_mrhs<DAG, R12, DOT, 1>), grid, dim3(256), 0, st, k, m); break;
    case 2: hipLaunchKernelGGL((wilson_mrhs<DAG, R12, DOT, 2>), grid, dim3(256), 0, st, k, m); break;
    case 3: hipLaunchKernelGGL((wilson_mrhs<DAG, R12, DOT, 3>), grid, dim3(256), 0, st, k, m); break;
    default: hipLaunchKernelGGL((wilson_mrhs<DAG, R12, DOT, 4>), grid, dim3(256), 0, st, k, m); break;
    }
}
template <bool DAG, bool R12>
static void mrhs_launch_dot(bool dot, int nb, dim3 grid, hipStream_t st, const KArgs& k, const MCols& m) {
    if (dot) mrhs_launch_nb<DAG, R12, true>(nb, grid, st, k, m);
    else mrhs_launch_nb<DAG, R12, false>(nb, grid, st, k, m);
}

}  // inline namespace (precision)

bool mrhs_applies(lqcd_op_s* op) {
    lqcd_ctx_s* c = op->ctx;
    return op->kind == LQCD_WILSON && op->r == 1.0 && !(op->csw != 0.0 && op->clover) && !any_partitioned(c) && !c->has_comm && c->nranks == 1 &&
           c->local_peers.empty() && c->geom.Vh % 64 == 0;
}

int mrhs_hop_launch(lqcd_op_s* op, const MrhsCall& s) {
    lqcd_ctx_s* c = op->ctx;
    if (!mrhs_applies(op) || s.n < 1 || s.n > LQCD_MRHS_MAX || s.parity_mode < 0 || s.parity_mode > 2) {
        set_error("stencil_mrhs: the multi-column hop needs the Wilson operator with r = 1, no clover term, an unpartitioned lattice of whole 64-site chunks and 1 .. LQCD_MRHS_MAX columns");
        return LQCD_ERR_UNSUPPORTED;
    }
    const bool dot = s.dot_partial[0] != nullptr;
    if (dot && s.parity_mode == 2) { set_error("stencil_mrhs: the dot epilogue runs on one parity"); return LQCD_ERR_UNSUPPORTED; }
    apply_bc(c, op->bc);
    // 12-real links while every link of the field passes the gate of the single-column kernels (fields.hip gauge_ensure_recon12), all 18 reals otherwise
    const bool r12 = c->tun.gauge_recon == 12 && gauge_ensure_recon12(op->gauge) == LQCD_OK && op->gauge->recon_ok;
    c->tun.recon_active = r12 ? 1 : 0;
    KArgs k = {};
    k.g = c->geom;
    k.gauge = op->gauge->data;
    k.gauge12 = r12 ? op->gauge->data12 : nullptr;
    k.a = s.a; k.b = s.b; k.r = 1.0;
    k.parity_mode = s.parity_mode;
    const BlockMap bm = make_block_map(c->geom, c->tun.xcd_remap, c->tun.xcd_nsub, c->tun.xcd_ysplit);      // the XCD-aware tile sweep of the single-column kernels
    k.nblocks = s.parity_mode == 2 ? bm.nblocks : bm.nblocks / 2;
    k.remap = bm.remap; k.cps = bm.cps; k.cpp = bm.cpp; k.ysplit = bm.ysplit; k.cpr = bm.cpr; k.ty = bm.ty; k.tz = bm.tz; k.nsub = 0;
    k.d_perpass = bm.d_perpass; k.d_cpr = bm.d_cpr; k.d_ysplit = bm.d_ysplit; k.d_ty = bm.d_ty;
    k.nt = c->tun.nt_store ? 4 : 0;
    c->tun.nt_active = k.nt;      // read-only key: plain link loads, no NTB instance
    const dim3 grid(k.nblocks);
    for (int j0 = 0; j0 < s.n; j0 += MR_NB) {
        const int nb = std::min(MR_NB, s.n - j0);
        MCols m = {};
        for (int q = 0; q < nb; q++) {
            for (int p = 0; p < 2; p++) { m.out[p][q] = s.out[p][j0 + q]; m.in[p][q] = s.in[p][j0 + q]; m.xin[p][q] = s.xin[p][j0 + q]; }
            m.z[q] = s.dot_z[j0 + q]; m.dot[q] = s.dot_partial[j0 + q]; m.done[q] = s.done[j0 + q];
        }
        m.conj = s.dot_conj;
        if (r12) { if (s.dagger) mrhs_launch_dot<true, true>(dot, nb, grid, c->stream, k, m); else mrhs_launch_dot<false, true>(dot, nb, grid, c->stream, k, m); }
        else { if (s.dagger) mrhs_launch_dot<true, false>(dot, nb, grid, c->stream, k, m); else mrhs_launch_dot<false, false>(dot, nb, grid, c->stream, k, m); }
        HIPCHK(hipGetLastError());
    }
    c->tun.mrhs_active = std::min(MR_NB, s.n);
    return LQCD_OK;
}

}  // namespace lqcd
