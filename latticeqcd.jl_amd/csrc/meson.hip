// meson.hip -- meson correlators from point-source propagators, contracted per time slice on the device.  Reference caller: the Pion_correlator measurement
// (src/measurements/unusedfiles/measure_Pion_correlator.jl: 12 (Wilson) or 3 (staggered) point-source solves in the icum order ic, is -- colour-major --, :376
// setindex_global!, :283 Cpi[t] += |S|^2).
//
// Definitions (directions 0..3 = x, y, z, t; gLt = the global time extent; gamma_mu, gamma_5 = the matrices the operator is built with, SURVEY.md Appendix A, each a
// permutation with phases in {+-1, +-i}):
//   Gamma_n = gamma_x^n0 gamma_y^n1 gamma_z^n2 gamma_t^n3,   n = n0 + 2 n1 + 4 n2 + 8 n3 = 0..15          (Gamma_15 = gamma_5 with these matrices)
//   S(x)[alpha a, beta b] = component (sink spin alpha, sink colour a) of the solution of D S = delta_{x,x0} delta_{alpha beta} delta_{ab}, x0 the global source site
//   C_n(t) = sum_{x: x_t = t} Re tr_{spin,colour}[ Gamma_n S(x) Gamma_n^+ gamma_5 S(x)^+ gamma_5 ],   t the absolute global time coordinate (the reference's Cpi[t])
// C_15(t) = sum |S|^2 is the reference's Pion_correlator; C_1 + C_2 + C_4 is the rho.  The trace splits over the colour pairs (a, b): with the 4 x 4 spin matrix
// M = S[. a, . b],  tr = sum_{a,b} tr_spin[ Gamma M (Gamma^+ gamma_5) M^+ gamma_5 ], and every factor but M is a phased permutation: 16 terms i^k M[a'][b'] conj(M[d][e]) per
// channel and colour pair, whose indices and k are generated at compile time (meson_term) -- every register index is static, the real part of a term is two FMAs.
//
// Kernels (one thread per site, launched over (256 sites of a time slice, t, parity): a time slice holds XH LY LZ sites per parity, which is a whole number of 64-site
// chunks only from 8 x 8 x 8 up, so a workgroup is confined to ONE slice and the lanes behind its end are masked -- no thread ever bins into a foreign t):
//   meson_contract_kernel   one source colour b: for every sink colour a the 16 numbers S[alpha a, beta b] from the four columns' component planes (16-byte coalesced
//                           loads, each column read once: 192 B per site and column), all 16 channels accumulated in registers; wave sums by DPP, the four wave sums
//                           of a workgroup through LDS in sequence, one partial per (channel, t, workgroup)
//   meson_norm2_kernel      the same binning for sum |s|^2 of one field (Wilson or staggered)
//   meson_final_kernel      one workgroup per (channel, t) adds the partials in a fixed order (strided per thread, then a tree) onto the device table at slot origin[3] + t
// The device table [16][gLt] is zero-filled first, so on a partitioned lattice one all-reduce of it gives every rank the whole table.  One device-to-host copy, at the
// end; no floating-point atomics anywhere: a table is bitwise reproducible call to call.
#include "ops_internal.h"

#include <utility>
#include <vector>

namespace lqcd {

constexpr int MS_THREADS = 256;
constexpr int MS_NCHAN = LQCD_MESON_NCHAN;

// a phased permutation matrix: row a has its one entry in column col[a], value i^ph[a]
struct PhPerm { int col[4]; int ph[4]; };
constexpr PhPerm pp_one() { return PhPerm{{0, 1, 2, 3}, {0, 0, 0, 0}}; }
constexpr PhPerm pp_gamma(int mu) {
    if (mu == 3) return PhPerm{{0, 1, 2, 3}, {0, 0, 2, 2}};
    return PhPerm{{PERM[mu][0], PERM[mu][1], PERM[mu][2], PERM[mu][3]}, {GK[mu][0], GK[mu][1], GK[mu][2], GK[mu][3]}};
}
constexpr PhPerm pp_mul(PhPerm A, PhPerm B) {
    PhPerm C = pp_one();
    for (int a = 0; a < 4; a++) { C.col[a] = B.col[A.col[a]]; C.ph[a] = (A.ph[a] + B.ph[A.col[a]]) & 3; }
    return C;
}
constexpr PhPerm pp_adj(PhPerm A) {
    PhPerm C = pp_one();
    for (int a = 0; a < 4; a++) { C.col[A.col[a]] = a; C.ph[A.col[a]] = (4 - A.ph[a]) & 3; }
    return C;
}
constexpr PhPerm pp_channel(int n) {
    PhPerm G = pp_one();
    for (int mu = 0; mu < 4; mu++)
        if ((n >> mu) & 1) G = pp_mul(G, pp_gamma(mu));
    return G;
}
constexpr PhPerm pp_gamma5() { return pp_channel(15); }      // gamma_5 = gamma_x gamma_y gamma_z gamma_t

// term T = 4 al + bp of tr[A M B M^+ C], A = Gamma_N, B = Gamma_N^+ gamma_5, C = gamma_5:
//   A[al][ap] M[ap][bp] B[bp][be] conj(M[de][be]) C[de][al]   with ap = A.col[al], be = B.col[bp], de the row of C whose entry sits in column al
template <int N, int T>
__device__ __forceinline__ void meson_term(double& acc, const cd (&M)[4][4]) {
    constexpr PhPerm A = pp_channel(N), Cm = pp_gamma5(), B = pp_mul(pp_adj(A), Cm), Ci = pp_adj(Cm);
    constexpr int al = T >> 2, bp = T & 3;
    constexpr int ap = A.col[al], be = B.col[bp], de = Ci.col[al];
    constexpr int k = (A.ph[al] + B.ph[bp] + Cm.ph[de]) & 3;
    const cd z = M[ap][bp], w = M[de][be];      // Re[i^k z conj(w)]
    if constexpr (k == 0) { acc = fma(z.re, w.re, acc); acc = fma(z.im, w.im, acc); }
    else if constexpr (k == 1) { acc = fma(z.re, w.im, acc); acc = fma(-z.im, w.re, acc); }
    else if constexpr (k == 2) { acc = fma(-z.re, w.re, acc); acc = fma(-z.im, w.im, acc); }
    else { acc = fma(z.im, w.re, acc); acc = fma(-z.re, w.im, acc); }
}
template <int N, int... T>
__device__ __forceinline__ void meson_channel(double& acc, const cd (&M)[4][4], std::integer_sequence<int, T...>) {
    (meson_term<N, T>(acc, M), ...);
}
template <int... N>
__device__ __forceinline__ void meson_channels(double (&acc)[MS_NCHAN], const cd (&M)[4][4], std::integer_sequence<int, N...>) {
    (meson_channel<N>(acc[N], M, std::make_integer_sequence<int, 16>{}), ...);
}

struct MesonArgs {
    Geom g;
    const double2* col[4];  // the four spin columns of one source colour (FULL Wilson fields), or col[0] = the field of the norm kernel
    double* partial;        // [channel][t][2 nbs]
    int slice;              // sites of a time slice per parity
    int nbs;                // workgroups per (time slice, parity)
};

// the site of this thread inside time slice blockIdx.y, parity blockIdx.z (a lane behind the end of the slice takes the slice's first site and contributes nothing)
__device__ __forceinline__ bool meson_site(const MesonArgs& k, int& cb) {
    const int j = blockIdx.x * MS_THREADS + threadIdx.x;
    const bool act = j < k.slice;
    cb = (int)blockIdx.y * k.slice + (act ? j : 0);
    return act;
}

// wave sums of nv values -> LDS -> thread v < nv adds the four wave sums in sequence and writes partial[v][t][workgroup]
template <int NV>
__device__ __forceinline__ void meson_block_out(const MesonArgs& k, const double (&v)[NV], bool act, double (&red)[MS_NCHAN][MS_THREADS / 64]) {
#pragma unroll
    for (int n = 0; n < NV; n++) {
        const double s = wave_sum(act ? v[n] : 0.0);
        if ((threadIdx.x & 63) == 0) red[n][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < NV) {
        const int n = threadIdx.x;
        const double s = ((red[n][0] + red[n][1]) + red[n][2]) + red[n][3];
        k.partial[((size_t)n * gridDim.y + blockIdx.y) * (2 * k.nbs) + (size_t)blockIdx.z * k.nbs + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(MS_THREADS) void meson_contract_kernel(MesonArgs k) {
    __shared__ double red[MS_NCHAN][MS_THREADS / 64];
    int cb;
    const bool act = meson_site(k, cb);
    const size_t off = (size_t)blockIdx.z * 12 * k.g.Vs + sp_off(12, cb);
    const int st = sp_stride(k.g);
    double acc[MS_NCHAN];
#pragma unroll
    for (int n = 0; n < MS_NCHAN; n++) acc[n] = 0.0;
#pragma unroll 1
    for (int a = 0; a < 3; a++) {       // sink colour
        cd M[4][4];                     // M[alpha][beta] = S[alpha a, beta b]
#pragma unroll
        for (int be = 0; be < 4; be++) {
            const double2* q = k.col[be] + off + (size_t)a * st;
#pragma unroll
            for (int al = 0; al < 4; al++) M[al][be] = ld(q + (size_t)(3 * al) * st);
        }
        meson_channels(acc, M, std::make_integer_sequence<int, MS_NCHAN>{});
    }
    meson_block_out<MS_NCHAN>(k, acc, act, red);
}

template <int NCOMP>
__global__ __launch_bounds__(MS_THREADS) void meson_norm2_kernel(MesonArgs k) {
    __shared__ double red[MS_NCHAN][MS_THREADS / 64];
    int cb;
    const bool act = meson_site(k, cb);
    const double2* q = k.col[0] + (size_t)blockIdx.z * NCOMP * k.g.Vs + sp_off(NCOMP, cb);
    const int st = sp_stride(k.g);
    cd z[NCOMP];
#pragma unroll
    for (int e = 0; e < NCOMP; e++) z[e] = ld(q + (size_t)e * st);      // all loads in flight, then the sum in component order
    double v[1] = {0.0};
#pragma unroll
    for (int e = 0; e < NCOMP; e++) {
        v[0] = fma(z[e].re, z[e].re, v[0]);
        v[0] = fma(z[e].im, z[e].im, v[0]);
    }
    meson_block_out<1>(k, v, act, red);
}

// workgroup (t, n): tab[n * gLt + t0 + t] += the sum of the np partials of (n, t), in a fixed order
__global__ __launch_bounds__(256) void meson_final_kernel(const double* __restrict__ partial, int np, double* __restrict__ tab, int gLt, int t0) {
    __shared__ double s[256];
    const double* q = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * np;
    double a = 0.0;
    for (int b = threadIdx.x; b < np; b += 256) a += q[b];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) tab[(size_t)blockIdx.y * gLt + t0 + blockIdx.x] += s[0];
}

static int ms_reserve(lqcd_ctx_s* c, double** buf, size_t* have, size_t n) {
    if (*have >= n) return LQCD_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)hipFree(*buf);
    *buf = nullptr; *have = 0;
    HIPCHK(hipMalloc((void**)buf, n * sizeof(double)));
    *have = n;
    return LQCD_OK;
}

static int ms_refuse_grid(lqcd_ctx_s* c, const char* who) {
    if (!c->local_peers.empty()) { set_error(std::string(who) + ": not available on an in-process PE grid"); return LQCD_ERR_UNSUPPORTED; }
    if (c->nranks > 1 && !c->has_comm) { set_error(std::string(who) + ": communicator not initialised (call lqcd_ctx_comm_init or lqcd_ctx_peer_init)"); return LQCD_ERR_ARG; }
    return LQCD_OK;
}

static MesonArgs ms_args(lqcd_ctx_s* c) {
    MesonArgs k;
    k.g = c->geom;
    k.slice = c->geom.XH * c->geom.L[1] * c->geom.L[2];
    k.nbs = (k.slice + MS_THREADS - 1) / MS_THREADS;
    k.partial = nullptr;
    for (int i = 0; i < 4; i++) k.col[i] = nullptr;
    return k;
}

// zero-filled device table of nchan rows
static int ms_begin(lqcd_ctx_s* c, int nchan) {
    HIPCHK(hipSetDevice(c->device));
    const MesonArgs k = ms_args(c);
    LQCHK(ms_reserve(c, &c->ms_partial, &c->ms_partial_n, (size_t)MS_NCHAN * c->geom.L[3] * 2 * k.nbs));
    LQCHK(ms_reserve(c, &c->ms_tab, &c->ms_tab_n, (size_t)MS_NCHAN * c->gL[3]));
    HIPCHK(hipMemsetAsync(c->ms_tab, 0, (size_t)nchan * c->gL[3] * sizeof(double), c->stream));
    return LQCD_OK;
}

// one colour block (four spin columns) onto the device table
static int ms_add_block(lqcd_ctx_s* c, lqcd_spinor_s* const* cols) {
    MesonArgs k = ms_args(c);
    for (int i = 0; i < 4; i++) k.col[i] = cols[i]->data;
    k.partial = c->ms_partial;
    const int Lt = c->geom.L[3];
    hipLaunchKernelGGL(meson_contract_kernel, dim3(k.nbs, Lt, 2), dim3(MS_THREADS), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(meson_final_kernel, dim3(Lt, MS_NCHAN), dim3(256), 0, c->stream, c->ms_partial, 2 * k.nbs, c->ms_tab, c->gL[3], c->geom.origin[3]);
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}

// sum |s|^2 per time slice of one field onto row 0 of the device table
static int ms_add_norm2(lqcd_ctx_s* c, lqcd_spinor_s* s) {
    MesonArgs k = ms_args(c);
    k.col[0] = s->data;
    k.partial = c->ms_partial;
    const int Lt = c->geom.L[3];
    if (s->ncomp == 12) hipLaunchKernelGGL(meson_norm2_kernel<12>, dim3(k.nbs, Lt, 2), dim3(MS_THREADS), 0, c->stream, k);
    else hipLaunchKernelGGL(meson_norm2_kernel<3>, dim3(k.nbs, Lt, 2), dim3(MS_THREADS), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(meson_final_kernel, dim3(Lt, 1), dim3(256), 0, c->stream, c->ms_partial, 2 * k.nbs, c->ms_tab, c->gL[3], c->geom.origin[3]);
    HIPCHK(hipGetLastError());
    return LQCD_OK;
}

// all-reduce of the device table over the ranks, the one copy to the host
static int ms_finish(lqcd_ctx_s* c, int nchan, double* out) {
    const int n = nchan * c->gL[3];
    if (c->has_comm) {
        if (c->peer.on) {       // the peer backend's reduction slots carry PEER_RED_VALS values at a time
            for (int o = 0; o < n; o += PEER_RED_VALS) LQCHK(comm_allreduce(c, c->ms_tab + o, n - o < PEER_RED_VALS ? n - o : PEER_RED_VALS));
        } else {
            LQCHK(comm_allreduce(c, c->ms_tab, n));
        }
    }
    std::vector<double> h(n);
    HIPCHK(hipMemcpyAsync(h.data(), c->ms_tab, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    LQCHK(comm_check(c));
    for (int j = 0; j < n; j++) out[j] = h[j];
    return LQCD_OK;
}

static bool ms_wilson_full(const lqcd_spinor_s* s) { return s && s->kind == LQCD_WILSON && s->subset == LQCD_FULL && s->ls == 1 && s->ncomp == 12; }

// the 12 solves + contraction of lqcd_meson_correlators; table and iters are written only when everything has succeeded
static int ms_wilson_correlators(lqcd_op_s* op, const int src[4], double eps, int maxiter, double* table, int* iters) {
    lqcd_ctx_s* c = op->ctx;
    ScratchScope pool(c);
    lqcd_spinor_s* b = pool.get(LQCD_WILSON, LQCD_FULL);
    lqcd_spinor_s* x[4];
    for (int is = 0; is < 4; is++) x[is] = pool.get(LQCD_WILSON, LQCD_FULL);
    if (!(b && x[0] && x[1] && x[2] && x[3])) { set_error("lqcd_meson_correlators: out of device memory"); return LQCD_ERR_HIP; }
    // tunable meson_mrhs = 1: the four spin columns of a source colour as ONE multi-column solve (four point sources resident instead of one); the contraction is unchanged
    const bool multi = c->tun.meson_mrhs != 0;
    lqcd_spinor_s* bm[4] = {b, nullptr, nullptr, nullptr};
    if (multi) {
        for (int is = 1; is < 4; is++) bm[is] = pool.get(LQCD_WILSON, LQCD_FULL);
        if (!(bm[1] && bm[2] && bm[3])) { set_error("lqcd_meson_correlators: out of device memory"); return LQCD_ERR_HIP; }
    }
    LQCHK(ms_begin(c, MS_NCHAN));
    int its[12];
    for (int ic = 0; ic < 3; ic++) {
        if (multi) {
            for (int is = 0; is < 4; is++) {
                LQCHK(lqcd_spinor_point_source(bm[is], src, ic, is));
                LQCHK(lqcd_spinor_zero(x[is]));
            }
            LQCHK(lqcd_solve_bicgstab_eo_multi(op, 4, x, bm, 0, eps, maxiter, &its[4 * ic], nullptr));
        } else {
            for (int is = 0; is < 4; is++) {
                LQCHK(lqcd_spinor_point_source(b, src, ic, is));
                LQCHK(lqcd_spinor_zero(x[is]));
                LQCHK(lqcd_solve_bicgstab_eo(op, x[is], b, 0, eps, maxiter, &its[4 * ic + is], nullptr));
            }
        }
        LQCHK(ms_add_block(c, x));
    }
    std::vector<double> t((size_t)MS_NCHAN * c->gL[3]);
    LQCHK(ms_finish(c, MS_NCHAN, t.data()));
    for (size_t j = 0; j < t.size(); j++) table[j] = t[j];
    if (iters) for (int j = 0; j < 12; j++) iters[j] = its[j];
    return LQCD_OK;
}

static int ms_check_op(lqcd_op_s* op, const int src[4], const void* out, const char* who, bool staggered_ok) {
    if (!(op && op->ctx && src && out)) { set_error(std::string(who) + ": null argument"); return LQCD_ERR_ARG; }
    lqcd_ctx_s* c = op->ctx;
    if (op->kind == LQCD_DOMAINWALL) { set_error(std::string(who) + ": not available for the Domainwall operator"); return LQCD_ERR_UNSUPPORTED; }
    if (op->kind == LQCD_STAGGERED && !staggered_ok) { set_error(std::string(who) + ": the 16 channels are defined for the Wilson and Wilson-clover operators (staggered: lqcd_pion_correlator)"); return LQCD_ERR_UNSUPPORTED; }
    LQCHK(ms_refuse_grid(c, who));
    for (int mu = 0; mu < 4; mu++)
        if (src[mu] < 0 || src[mu] >= c->gL[mu]) { set_error(std::string(who) + ": source site outside the global lattice"); return LQCD_ERR_ARG; }
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

extern "C" int lqcd_spinor_norm2_timeslices(lqcd_spinor_t s, double* out) {
    ARGCHK(s && s->ctx && out, "lqcd_spinor_norm2_timeslices: null argument");
    ARGCHK(s->subset == LQCD_FULL && s->ls == 1 && (s->kind == LQCD_WILSON || s->kind == LQCD_STAGGERED), "lqcd_spinor_norm2_timeslices: need a FULL four-dimensional Wilson or staggered field");
    lqcd_ctx_s* c = s->ctx;
    LQCHK(ms_refuse_grid(c, "lqcd_spinor_norm2_timeslices"));
    LQCHK(ms_begin(c, 1));
    LQCHK(ms_add_norm2(c, s));
    return ms_finish(c, 1, out);
}

extern "C" int lqcd_meson_contract(const lqcd_spinor_t* cols, int ncol, double* table) {
    ARGCHK(cols && table, "lqcd_meson_contract: null argument");
    ARGCHK(ncol == 4 || ncol == 8 || ncol == 12, "lqcd_meson_contract: ncol = 4, 8 or 12 (whole colour blocks of four spin columns)");
    for (int j = 0; j < ncol; j++) {
        ARGCHK(cols[j], "lqcd_meson_contract: null column");
        ARGCHK(ms_wilson_full(cols[j]) && cols[j]->ctx && cols[j]->ctx == cols[0]->ctx, "lqcd_meson_contract: the columns must be FULL Wilson fields of one context");
    }
    lqcd_ctx_s* c = cols[0]->ctx;
    LQCHK(ms_refuse_grid(c, "lqcd_meson_contract"));
    LQCHK(ms_begin(c, MS_NCHAN));
    for (int b = 0; b < ncol / 4; b++) LQCHK(ms_add_block(c, cols + 4 * b));
    return ms_finish(c, MS_NCHAN, table);
}

extern "C" int lqcd_meson_correlators(lqcd_op_t op, const int src[4], double eps, int maxiter, double* table, int* iters) {
    LQCHK(ms_check_op(op, src, table, "lqcd_meson_correlators", false));
    return ms_wilson_correlators(op, src, eps, maxiter, table, iters);
}

extern "C" int lqcd_pion_correlator(lqcd_op_t op, const int src[4], double eps, int maxiter, double* C, int* iters) {
    LQCHK(ms_check_op(op, src, C, "lqcd_pion_correlator", true));
    lqcd_ctx_s* c = op->ctx;
    const int gLt = c->gL[3];
    if (op->kind == LQCD_WILSON) {      // row 15 of the 16-channel table: the same launches, so the same bits
        std::vector<double> t((size_t)MS_NCHAN * gLt);
        LQCHK(ms_wilson_correlators(op, src, eps, maxiter, t.data(), iters));
        for (int j = 0; j < gLt; j++) C[j] = t[(size_t)15 * gLt + j];
        return LQCD_OK;
    }
    // staggered: G = D^-1 delta = D^+ (D^+D)^-1 delta for the three source colours, C(t) = sum |G|^2
    ScratchScope pool(c);
    lqcd_spinor_s *b = pool.get(LQCD_STAGGERED, LQCD_FULL), *y = pool.get(LQCD_STAGGERED, LQCD_FULL), *x = pool.get(LQCD_STAGGERED, LQCD_FULL);
    if (!(b && y && x)) { set_error("lqcd_pion_correlator: out of device memory"); return LQCD_ERR_HIP; }
    LQCHK(ms_begin(c, 1));
    int its[3];
    for (int ic = 0; ic < 3; ic++) {
        LQCHK(lqcd_spinor_point_source(b, src, ic, 0));
        LQCHK(lqcd_spinor_zero(y));
        LQCHK(lqcd_solve_cg_DdagD(op, y, b, eps, maxiter, &its[ic], nullptr));
        LQCHK(lqcd_op_apply(op, x, y, 1));
        LQCHK(ms_add_norm2(c, x));
    }
    std::vector<double> t(gLt);
    LQCHK(ms_finish(c, 1, t.data()));
    for (int j = 0; j < gLt; j++) C[j] = t[j];
    if (iters) for (int j = 0; j < 3; j++) iters[j] = its[j];
    return LQCD_OK;
}
