// gauge_staple.h -- what the units of the gauge side share (staple.hip, md.hip, links.hip, stout.hip, heatbath.hip, flow.hip, clover.hip).  Device part: 3x3 link
// algebra, link loads, the forward-ghost / lower-staple reads of a partitioned lattice, the traceless anti-Hermitian projection, exp and the projection back onto
// SU(3) -- every helper defined once, before its first use.  Host part (end of the file): the functions one of these units offers to the others.
#pragma once
#include "lqcd_internal.h"

#include <string>

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
// two thirds of the bytes through the L1 / L2 path, which is what bounds the staple sweep (60 neighbour-link loads per site).
// load_u_raw: rows 0, 1 as they come from memory; finish_u: row 2 rebuilt, for a link or for rows 0, 1 of a product of links
__device__ __forceinline__ void load_u_raw(cd (&u)[9], const double2* __restrict__ base, int stride) {
#pragma unroll
    for (int e = 0; e < 6; e++) u[e] = ld(base + (size_t)e * stride);
}
__device__ __forceinline__ void finish_u(cd (&u)[9]) {
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const int b1 = (b + 1) % 3, b2 = (b + 2) % 3;
        const cd x = cmul(u[b1], u[3 + b2]) - cmul(u[b2], u[3 + b1]);
        u[6 + b] = mk(x.re, -x.im);
    }
}
template <bool R2>
__device__ __forceinline__ void load_u(cd (&u)[9], const double2* __restrict__ base, int stride) {
    if constexpr (!R2) { load_m3(u, base, stride); return; }
    load_u_raw(u, base, stride);
    finish_u(u);
}
__device__ __forceinline__ void store_m3(double2* base, int stride, const cd (&a)[9]) {
#pragma unroll
    for (int e = 0; e < 9; e++) st(base + (size_t)e * stride, a[e]);
}
__device__ __forceinline__ void dag3(cd (&o)[9], const cd (&a)[9]) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) o[r * 3 + q] = mk(a[q * 3 + r].re, -a[q * 3 + r].im);
}
__device__ __forceinline__ void add3(cd (&o)[9], const cd (&a)[9]) {
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = o[k] + a[k];
}
__device__ __forceinline__ void sub3(cd (&o)[9], const cd (&a)[9]) {
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = o[k] - a[k];
}
// x = 2 h TA(w),  TA(w) = (w - w^+)/2 - tr(w - w^+)/6: the caller's scale enters as ONE factor h on the differences (h = 0.5: TA itself), the trace goes last
__device__ __forceinline__ void ta3(cd (&x)[9], const cd (&w)[9], double h) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) x[r * 3 + q] = mk(h * (w[r * 3 + q].re - w[q * 3 + r].re), h * (w[r * 3 + q].im + w[q * 3 + r].im));
    const double tr = (x[0].im + x[4].im + x[8].im) / 3.0;    // the anti-Hermitian part has an imaginary trace
    x[0].im -= tr; x[4].im -= tr; x[8].im -= tr;
}
// max-abs-row-sum norm
__device__ __forceinline__ double rowsum_norm(const cd (&x)[9]) {
    double nrm = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++)
        nrm = fmax(nrm, (fabs(x[a * 3].re) + fabs(x[a * 3].im)) + (fabs(x[a * 3 + 1].re) + fabs(x[a * 3 + 1].im)) + (fabs(x[a * 3 + 2].re) + fabs(x[a * 3 + 2].im)));
    return nrm;
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
    finish_u(u);
}

// exp(dt P).  Below max-abs-row-sum norm 2 of X = dt P (an MD step has a few 1e-2) the Taylor series is summed through the Cayley-Hamilton identity
// X^3 = t X^2 - s X + d I (t = tr X, s = (t^2 - tr X^2)/2, d = det X; true for every 3x3 matrix, nothing assumed about P): X^n = al_n I + be_n X + ga_n X^2
// with the scalar recurrence al' = d ga, be' = al - s ga, ga' = be + t ga, so exp X = a0 I + a1 X + a2 X^2 costs ONE matrix product and a dozen scalar
// steps instead of a matrix product per term (r04: the link update inside the staple sweep is ALU time, 1.78 -> 1.63 ms already from a shorter series).
// Terms: until nrm^(n+1)/(n+1)! < 1e-18, two more for the n^2 growth of the coefficients (<= 6e-16 from scipy's expm up to norm 2, near-degenerate spectra included).
// Norm >= 2: the Taylor series in Horner form.  (stout.hip's exp_any3 is this tail with its own term table: sharing its text reschedules link_op_kernel<1>.)
__device__ __forceinline__ void exp_m3(cd (&e)[9], cd (&x)[9], double dt) {     // e = exp(dt x); x is scaled in place
#pragma unroll
    for (int k = 0; k < 9; k++) x[k] = mk(dt * x[k].re, dt * x[k].im);
    cd t[9];
    const double nrm = rowsum_norm(x);
    if (nrm < 2.0) {
        const int nt = (nrm < 0.009 ? 6 : nrm < 0.04 ? 8 : nrm < 0.11 ? 10 : nrm < 0.2 ? 12 : nrm < 0.5 ? 16 : nrm < 1.0 ? 20 : 28) + 2;
        mm3(t, x, x);
        const cd tr = x[0] + x[4] + x[8], tr2 = t[0] + t[4] + t[8], trtr = cmul(tr, tr);
        const cd s = mk(0.5 * (trtr.re - tr2.re), 0.5 * (trtr.im - tr2.im));
        const cd d = cmul(x[0], cmul(x[4], x[8]) - cmul(x[5], x[7])) - cmul(x[1], cmul(x[3], x[8]) - cmul(x[5], x[6])) +
                     cmul(x[2], cmul(x[3], x[7]) - cmul(x[4], x[6]));
        cd al = mk(1.0, 0.0), be = mk(0.0, 0.0), ga = mk(0.0, 0.0), a0 = al, a1 = be, a2 = ga;
        double f = 1.0;
        for (int n = 1; n <= nt; n++) {
            const cd al2 = cmul(d, ga), be2 = al - cmul(s, ga), ga2 = be + cmul(tr, ga);
            al = al2; be = be2; ga = ga2;
            f /= (double)n;
            a0 = mk(fma(f, al.re, a0.re), fma(f, al.im, a0.im));
            a1 = mk(fma(f, be.re, a1.re), fma(f, be.im, a1.im));
            a2 = mk(fma(f, ga.re, a2.re), fma(f, ga.im, a2.im));
        }
#pragma unroll
        for (int k = 0; k < 9; k++) {
            e[k] = cmul(a1, x[k]) + cmul(a2, t[k]);
            if (k % 4 == 0) e[k] = e[k] + a0;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 9; k++) e[k] = mk((k % 4 == 0) ? 1.0 : 0.0, 0.0);
    for (int n = nrm < 4.0 ? 36 : 60; n >= 1; n--) {
        mm3(t, x, e);
        const double inv = 1.0 / (double)n;
#pragma unroll
        for (int k = 0; k < 9; k++) e[k] = mk(((k % 4 == 0) ? 1.0 : 0.0) + inv * t[k].re, inv * t[k].im);
    }
}
// only a link that IS on the group up to accumulated rounding (deviation <= 1e-13) is put back onto it: the projection then moves it by
// about that rounding.  A configuration read from a text file (the reference's fixtures are unitary to 9e-11) is left exactly as the
// reference's literal update leaves it.
__device__ __forceinline__ void project_if_on_group(cd (&t)[9], unsigned* notproj) {
    cd v[9];
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = t[k];
    reunitarize_m3(v);
    double dev = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) dev = fmax(dev, fmax(fabs(v[k].re - t[k].re), fabs(v[k].im - t[k].im)));
    if (dev <= 1e-13) {
#pragma unroll
        for (int k = 0; k < 9; k++) t[k] = v[k];
    } else {
        *notproj = 1u;      // some link of this field is not on the group (benign race: every writer stores the same value)
    }
}

// whole-field kernels, one thread per link: workgroup = 64 consecutive sites of one parity x 4 waves (wave = mu), every access of a wave is one
// contiguous 1 KiB run of the chunk-blocked layout; grid = link_grid
__device__ __forceinline__ bool link_of_thread(const Geom& g, size_t& off) {
    const int p = blockIdx.x & 1, i = (blockIdx.x >> 1) * 64 + (threadIdx.x & 63), mu = threadIdx.x >> 6;
    if (i >= g.Vh) return false;
    off = glink_off(g, p, mu, i);
    return true;
}
// single-direction kernels: one 64-thread block per 64 sites of one parity (the same grid)
__device__ __forceinline__ bool site_of_thread(const Geom& g, int& p, int& i) {
    p = blockIdx.x & 1; i = (blockIdx.x >> 1) * 64 + threadIdx.x;
    return i < g.Vh;
}
inline int link_grid(const Geom& g) { return 2 * g.nch; }

// ---------------------------------------------------------------------------------- host side: what one unit offers to the others
inline int same_ctx(lqcd_gauge_t a, lqcd_gauge_t b, const char* who) {
    if (!(a && b && a->ctx == b->ctx && a != b)) { set_error(std::string(who) + ": need two distinct gauge-shaped fields of one context"); return LQCD_ERR_ARG; }
    return LQCD_OK;
}
// The md_reunitarize flag protocol around ONE launch that may project links back onto the group: the device word is cleared, `launch(flag)` enqueues the kernel,
// the word comes back and the stream is waited for.  *all_projected: reunit was asked for and no link was left off the group.
template <class Launch>
int launch_with_notproj_flag(lqcd_ctx_s* c, bool reunit, bool* all_projected, Launch&& launch) {
    unsigned* flag = c->pipe_ctr + PIPE_CTR_NOTPROJ_WORD;      // a spare word of the counter block
    unsigned notproj = 1;
    if (reunit) HIPCHK(hipMemsetAsync(flag, 0, sizeof(unsigned), c->stream));
    launch(flag);
    HIPCHK(hipGetLastError());
    if (reunit) HIPCHK(hipMemcpyAsync(&notproj, flag, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *all_projected = reunit && !notproj;
    return LQCD_OK;
}

// staple.hip
int gauge_halo_links(lqcd_gauge_s* U);      // partitioned lattice: the x_lam = 0 link slices of U travel to the -lam neighbours (forward ghosts, c->gf_ghost); enqueued
int gf_exchange_rccl(lqcd_ctx_s* c, double2* const sendb[4], double2* const recvb[4], bool to_backward);      // grouped send / recv of buffers of 4 matrices per face site
int staple_halo_args(lqcd_gauge_s* U, GFArgs& k);
int staple_force(lqcd_gauge_s* out, lqcd_gauge_s* U, double beta, double factor, bool fuse, int mu_only = -1, int mu_out = 0, double coef_override = 0.0);
int staple_force_expu(lqcd_gauge_s* P, lqcd_gauge_s* U, double beta, double factor, double dt);
int flow_stage(lqcd_gauge_s* U, double2* X, double xscale, double factor, bool xread, unsigned* notproj, bool two_rows);
// md.hip
int link_exp_update_enqueue(lqcd_gauge_s* U, double dt, const double2* P, bool reunit, unsigned* notproj);      // U <- exp(dt P) U, launch only
int gauge_exp_update_now(lqcd_gauge_t U, double dt, lqcd_gauge_t P);
// fields.hip, clover.hip
int plaquette_local_sum_device(lqcd_gauge_s* g, const double2* const ghost[4], double* d_sum);
int gauge_ext_links(lqcd_ctx_s* c, const lqcd_gauge_s* U, const double2** ext, int E[4], size_t* n);

}  // namespace lqcd
