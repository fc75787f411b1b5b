// links.hip -- the per-direction link operations the reference's unchanged callers ask for (U[mu], p[mu], one temporary link field at a time:
// src/md/AbstractMD.jl:78-135), their lqcd_link_* entry points, and the recorder that turns the callers' call triples back into fused launches ("lazy link
// triples" below: pure host logic).  The fused four-direction kernels the recorder ends in are staple.hip (staple_force, staple_force_expu) and md.hip
// (gauge_exp_update_now); conventions: md.hip header.
#include "lqcd_internal.h"
#include "gauge_staple.h"

#include <vector>

namespace lqcd {

// ---- single-direction forms: one 64-thread block per 64 sites of one parity, the direction slots are arguments.  They serve the
// reference's callers literally; the fused four-direction kernels remain the fast path.
// op 0: C = t A (substitute_U! with t = 1)   op 1: C = exp(t A) (exptU!)   op 2: C = A B (mul!)   op 3: C += t * TA(A) (Traceless_antihermitian_add!)
template <int OP>
// C, A and B may be slots of one allocation, and C may be A or B itself (substitute_U!(U, U), mul!(temp1, U[mu], dSdUmu) on slots of one
// storage): no __restrict__ -- every thread loads all of its inputs before it stores, which is what makes the in-place forms well defined
__global__ __launch_bounds__(64) void link_op_kernel(Geom g, double2* C, int mc, const double2* A, int ma, const double2* B, int mb, double t, unsigned* notproj) {
    int p, i;
    if (!site_of_thread(g, p, i)) return;
    const int Gs = glink_stride(g);
    cd a[9], r[9];
    load_m3(a, A + glink_off(g, p, ma, i), Gs);
    double2* o = C + glink_off(g, p, mc, i);
    if constexpr (OP == 0) {
#pragma unroll
        for (int e = 0; e < 9; e++) r[e] = mk(t * a[e].re, t * a[e].im);
    } else if constexpr (OP == 1) {
        exp_m3(r, a, t);
    } else if constexpr (OP == 2) {
        cd b[9];
        load_m3(b, B + glink_off(g, p, mb, i), Gs);
        mm3(r, a, b);
    } else if constexpr (OP == 6) {                 // A^+ B: mul!(dSdU[mu], Uout[mu]', UdSfdU[mu]) (standardMD.jl:211)
        cd b[9];
        load_m3(b, B + glink_off(g, p, mb, i), Gs);
        mm3_dn(r, a, b);
    } else if constexpr (OP == 4 || OP == 5) {      // exp(t A) B: exptU! + mul! of the reference's U_update! in one pass (C may be B: the in-place link update)
        cd e[9], b[9];
        exp_m3(e, a, t);
        load_m3(b, B + glink_off(g, p, mb, i), Gs);
        mm3(r, e, b);
        if constexpr (OP == 5) project_if_on_group(r, notproj);      // the projection rule of link_exp_update_kernel<true>
    } else {
        cd h[9];
        ta3(h, a, 0.5);
#pragma unroll
        for (int e = 0; e < 9; e++) {
            const cd pv = ld(o + (size_t)e * Gs);
            r[e] = mk(fma(t, h[e].re, pv.re), fma(t, h[e].im, pv.im));
        }
    }
#pragma unroll
    for (int e = 0; e < 9; e++) st(o + (size_t)e * Gs, r[e]);
}

// ---- single-direction entry points (the interface the reference's unchanged callers use, AbstractMD.jl:78-135)
static int link_args(lqcd_gauge_t a, int ma, lqcd_gauge_t b, int mb, const char* who) {
    if (!(a && b && a->ctx == b->ctx && ma >= 0 && ma < 4 && mb >= 0 && mb < 4)) {
        set_error(std::string(who) + ": need gauge-shaped fields of one context and direction slots in 0..3");
        return LQCD_ERR_ARG;
    }
    return LQCD_OK;
}
template <int OP>
static int link_op(lqcd_gauge_t C, int mc, lqcd_gauge_t A, int ma, lqcd_gauge_t B, int mb, double t) {
    lqcd_ctx_s* c = C->ctx;
    HIPCHK(hipSetDevice(c->device));
    C->version++;
    hipLaunchKernelGGL(link_op_kernel<OP>, dim3(link_grid(c->geom)), dim3(64), 0, c->stream, c->geom, C->data, mc, A->data, ma,
                       B ? B->data : (const double2*)nullptr, mb, t, c->pipe_ctr + PIPE_CTR_NOTPROJ_WORD);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return LQCD_OK;
}
// The three per-direction calls of the reference's U_update! (AbstractMD.jl:91-93) -- exptU!(expU, t, p[mu]); mul!(W, expU, U[mu]);
// substitute_U!(U[mu], W) -- as ONE pass: W[mu_w] = exp(t P[mu_p]) U[mu_u], W = U allowed (the in-place update of one direction).  Reached by
// the lazy triples below, or directly.  In place and with the tunable
// md_reunitarize the updated links are projected back onto SU(3) under the rule of lqcd_gauge_exp_update (the field stays "on the group" if it was).
static int link_exp_mul_now(lqcd_gauge_t W, int mu_w, double t, lqcd_gauge_t P, int mu_p, lqcd_gauge_t U, int mu_u) {
    lqcd_ctx_s* c = W->ctx;
    const bool inplace = W == U && mu_w == mu_u;
    if (!(inplace && c->tun.md_reunitarize)) return link_op<4>(W, mu_w, P, mu_p, U, mu_u, t);
    HIPCHK(hipSetDevice(c->device));
    const bool was_on_group = U->unitary_version == U->version;
    bool all_projected;
    LQCHK(launch_with_notproj_flag(c, true, &all_projected, [&](unsigned* flag) {
        U->version++;
        hipLaunchKernelGGL(link_op_kernel<5>, dim3(link_grid(c->geom)), dim3(64), 0, c->stream, c->geom, U->data, mu_w, P->data, mu_p, U->data, mu_u, t, flag);
    }));
    if (was_on_group && all_projected) U->unitary_version = U->version;      // the other three directions were on the group, this one was projected
    return LQCD_OK;
}

// ---- lazy link triples.  The reference's unchanged U_update! / P_update! (AbstractMD.jl:89-93, 107-111) update links and momenta one direction at a
// time through three generics each:
//     exptU!(expU, t, p[mu]);  mul!(W, expU, U[mu]);  substitute_U!(U[mu], W)                       -> lqcd_link_exp, lqcd_link_mul, lqcd_link_copy
//     calc_dSdUmu!(dSdUmu, ga, mu, U);  mul!(temp1, U[mu], dSdUmu);  Traceless_antihermitian_add!(p[mu], factor, temp1)
//                                                                                                  -> lqcd_link_staple, lqcd_link_mul, lqcd_link_add_ta
// The context RECORDS the first two calls of such a triple and launches ONE fused kernel at the third (link_exp_mul_now / link_add_ta_staple_now);
// completed triples are deferred once more, and when the same update has been asked for all four directions (what U_update! / P_update! do) the four
// become ONE launch of the fused four-direction kernel -- 1 launch per update instead of 12, callers and bindings unchanged (one ccall per generic).
// Every other entry point that reads, writes or destroys a gauge-shaped field (or applies an operator built on one) calls links_flush first, which
// runs what is recorded with the plain single-direction kernels in the order it was asked for: a temporary that IS read holds what the eager call
// would have put there.  The temporaries of a COMPLETED fused triple (expU, W / dSdUmu, temp1) are never written -- the reference's callers hand them
// back to their pool unread (unused!, AbstractMD.jl:95-97,113-117); a caller that does read them sets the tunable lazy_links = 0.
// In-process PE grids (lqcd_ctx_link_local, tests) run eagerly: their collectives are issued through lqcd_mdom_*.
static bool lazy_on(lqcd_ctx_s* c) { return c->tun.lazy_links && c->local_peers.empty(); }
static LinkRef lref(lqcd_gauge_s* g, int mu) { LinkRef r; r.g = g; r.mu = mu; return r; }

static int lazy_run_done(lqcd_ctx_s* c) {
    // waiting complete updates are older than every deferred triple; a momentum update is older than the link update behind it
    if (c->lazy.has_pp) {
        const LazyLinks::Done q = c->lazy.pp, r = c->lazy.pend;
        const bool both = c->lazy.has_pend && r.F == q.G && r.G == q.F && c->tun.lazy_merge > 1;
        c->lazy.has_pp = false;
        if (both) {
            c->lazy.has_pend = false;
            LQCHK(staple_force_expu(q.F, q.G, q.b, q.a, r.a));
        } else LQCHK(staple_force(q.F, q.G, q.b, q.a, true));
    }
    if (c->lazy.has_pend) {
        const LazyLinks::Done r = c->lazy.pend;
        c->lazy.has_pend = false;
        LQCHK(gauge_exp_update_now(r.F, r.a, r.G));
    }
    std::vector<LazyLinks::Done> d;
    d.swap(c->lazy.done);
    for (const LazyLinks::Done& r : d) {
        if (r.kind == 1) LQCHK(link_exp_mul_now(r.F, r.slot, r.a, r.G, r.slot, r.F, r.slot));
        else LQCHK(staple_force(r.F, r.G, r.b, r.a, true, r.slot, r.slot, 0.5 * r.b));
    }
    return LQCD_OK;
}
// a complete link update U <- exp(dt P) U: waits for a second one to merge with (tunable lazy_merge), or runs now
static int lazy_full_update(lqcd_ctx_s* c, lqcd_gauge_t U, double dt, lqcd_gauge_t P) {
    LazyLinks& z = c->lazy;
    if (!c->tun.lazy_merge) {
        if (z.has_pend || z.has_pp) LQCHK(lazy_run_done(c));
        return gauge_exp_update_now(U, dt, P);
    }
    if (z.has_pend && z.pend.F == U && z.pend.G == P) { z.pend.a += dt; return LQCD_OK; }
    if (z.has_pend || (z.has_pp && !(z.pp.F == P && z.pp.G == U))) LQCHK(lazy_run_done(c));
    const LazyLinks::Done d = {1, U, 0, dt, P, 0.0};
    z.pend = d;
    z.has_pend = true;
    return LQCD_OK;
}
// a complete momentum update P += factor TA(-(beta/6) U staples): everything that waits runs first (it reads the links); on one GPU it then waits itself
// for the link update that follows it (lazy_merge = 2: staple_force_expu)
static int lazy_full_pupdate(lqcd_ctx_s* c, lqcd_gauge_t P, double factor, lqcd_gauge_t U, double beta) {
    LazyLinks& z = c->lazy;
    if (z.has_pend || z.has_pp) LQCHK(lazy_run_done(c));
    if (c->tun.lazy_merge < 2 || any_partitioned(c) || P == U) return staple_force(P, U, beta, factor, true);
    const LazyLinks::Done d = {2, P, 0, factor, U, beta};
    z.pp = d;
    z.has_pp = true;
    return LQCD_OK;
}
// a completed triple: one of (up to) four of the same update, or run on its own
static int lazy_defer(lqcd_ctx_s* c, const LazyLinks::Done& r) {
    std::vector<LazyLinks::Done>& done = c->lazy.done;
    if (!done.empty()) {
        const LazyLinks::Done& d = done[0];
        bool clash = d.kind != r.kind || d.F != r.F || d.G != r.G || d.a != r.a || d.b != r.b;
        for (const LazyLinks::Done& e : done) clash = clash || e.slot == r.slot;
        if (clash) LQCHK(lazy_run_done(c));
    }
    {
        const LazyLinks& z = c->lazy;
        const bool wait_ok = r.kind == 1 && (!z.has_pend || (r.F == z.pend.F && r.G == z.pend.G)) && (!z.has_pp || (r.F == z.pp.G && r.G == z.pp.F));
        if ((z.has_pend || z.has_pp) && !wait_ok) LQCHK(lazy_run_done(c));
    }
    done.push_back(r);
    if (done.size() == 4) {
        done.clear();
        if (r.kind == 1) return lazy_full_update(c, r.F, r.a, r.G);
        return lazy_full_pupdate(c, r.F, -3.0 * r.a, r.G, r.b);      // factor TA(U (beta/2) staples) = (-3 factor) TA(-(beta/6) U staples)
    }
    return LQCD_OK;
}
// a new triple starts: an interrupted one runs first; deferred triples of the same kind stay deferred unless the new one writes one of their fields
static int lazy_open_triple(lqcd_ctx_s* c, int kind, const lqcd_gauge_s* tmp) {
    if (c->lazy.kind) return links_flush(c);
    bool run = (c->lazy.has_pend && (kind != 1 || c->lazy.pend.F == tmp || c->lazy.pend.G == tmp)) ||
               (c->lazy.has_pp && (kind != 1 || c->lazy.pp.F == tmp || c->lazy.pp.G == tmp));
    if (!c->lazy.done.empty()) {
        run = run || c->lazy.done[0].kind != kind;
        for (const LazyLinks::Done& e : c->lazy.done) run = run || e.F == tmp || e.G == tmp;
    }
    return run ? lazy_run_done(c) : LQCD_OK;
}
int links_flush(lqcd_ctx_s* c) {
    if (c->lazy.has_pend || c->lazy.has_pp || !c->lazy.done.empty()) LQCHK(lazy_run_done(c));
    LazyLinks z = c->lazy;
    c->lazy.kind = 0;
    if (z.kind == 1 || z.kind == 2) {
        LQCHK(link_op<1>(z.E.g, z.E.mu, z.P.g, z.P.mu, nullptr, 0, z.t));
        if (z.kind == 2) LQCHK(link_op<2>(z.W.g, z.W.mu, z.E.g, z.E.mu, z.U.g, z.U.mu, 0.0));
    } else if (z.kind == 3 || z.kind == 4) {
        LQCHK(staple_force(z.S.g, z.Ug, z.beta, 0.0, false, z.mu, z.S.mu, 0.5 * z.beta));
        if (z.kind == 4) LQCHK(link_op<2>(z.T.g, z.T.mu, z.Ug, z.mu, z.S.g, z.S.mu, 0.0));
    }
    return LQCD_OK;
}

}  // namespace lqcd

using namespace lqcd;

// substitute_U!(U[mu], W) (AbstractMD.jl:93): one direction of dst <- one direction of src (the same field is allowed).  Third call of the
// U_update! triple: U[mu] <- exp(t p[mu]) U[mu] in one pass
extern "C" int lqcd_link_copy(lqcd_gauge_t dst, int mu_dst, lqcd_gauge_t src, int mu_src) {
    LQCHK(link_args(dst, mu_dst, src, mu_src, "lqcd_link_copy"));
    lqcd_ctx_s* c = dst->ctx;
    LazyLinks& z = c->lazy;
    if (z.kind == 2 && z.W.is(src, mu_src) && z.U.is(dst, mu_dst) && z.P.g != dst) {
        const LazyLinks r = z;
        z.kind = 0;
        if (r.P.mu == mu_dst) {      // p[mu] with U[mu]: maybe one of four
            LazyLinks::Done d = {1, dst, mu_dst, r.t, r.P.g, 0.0};
            return lazy_defer(c, d);
        }
        if (c->lazy.has_pend || c->lazy.has_pp) LQCHK(lazy_run_done(c));
        return link_exp_mul_now(dst, mu_dst, r.t, r.P.g, r.P.mu, dst, mu_dst);
    }
    LQCHK(links_flush_of(c));
    if (dst == src && mu_dst == mu_src) return LQCD_OK;
    return link_op<0>(dst, mu_dst, src, mu_src, nullptr, 0, 1.0);
}
// dst[mu_dst] = s * src[mu_src]: hands one direction of a force field to the reference's caller in ITS sign convention
// (calc_UdSfdU! fills "U dS_f/dU" = -G, P_update_fermion! adds factor = -eps dtau times its TA part: AbstractMD.jl:127-132)
extern "C" int lqcd_link_scaled_copy(lqcd_gauge_t dst, int mu_dst, double s, lqcd_gauge_t src, int mu_src) {
    LQCHK(link_args(dst, mu_dst, src, mu_src, "lqcd_link_scaled_copy"));
    LQCHK(links_flush_of(dst));
    return link_op<0>(dst, mu_dst, src, mu_src, nullptr, 0, s);
}
// exptU!(expU, t, p[mu], temps) (AbstractMD.jl:91): E[mu_e] = exp(t P[mu_p]), the Taylor-Horner series of lqcd_gauge_exp_update.  First call of the
// U_update! triple: recorded
extern "C" int lqcd_link_exp(lqcd_gauge_t E, int mu_e, double t, lqcd_gauge_t P, int mu_p) {
    LQCHK(link_args(E, mu_e, P, mu_p, "lqcd_link_exp"));
    lqcd_ctx_s* c = E->ctx;
    if (lazy_on(c) && E != P) {
        LQCHK(lazy_open_triple(c, 1, E));      // p[mu] is only read, by this triple and by the deferred ones
        LazyLinks& z = c->lazy;
        z.kind = 1; z.E = lref(E, mu_e); z.P = lref(P, mu_p); z.t = t;
        return LQCD_OK;
    }
    LQCHK(links_flush_of(c));
    return link_op<1>(E, mu_e, P, mu_p, nullptr, 0, t);
}
// mul!(W, expU, U[mu]) / mul!(temp1, U[mu], dSdUmu) (AbstractMD.jl:92,109): C[mu_c](n) = A[mu_a](n) B[mu_b](n), site by site.  Second call of
// either triple: recorded
extern "C" int lqcd_link_mul(lqcd_gauge_t C, int mu_c, lqcd_gauge_t A, int mu_a, lqcd_gauge_t B, int mu_b) {
    LQCHK(link_args(C, mu_c, A, mu_a, "lqcd_link_mul"));
    LQCHK(link_args(C, mu_c, B, mu_b, "lqcd_link_mul"));
    lqcd_ctx_s* c = C->ctx;
    LazyLinks& z = c->lazy;
    if (z.kind == 1 && z.E.is(A, mu_a) && !z.E.is(C, mu_c) && !z.P.is(C, mu_c)) {
        z.kind = 2; z.W = lref(C, mu_c); z.U = lref(B, mu_b);
        return LQCD_OK;
    }
    if (z.kind == 3 && z.S.is(B, mu_b) && A == z.Ug && mu_a == z.mu && !z.S.is(C, mu_c) && C != z.Ug) {
        z.kind = 4; z.T = lref(C, mu_c);
        return LQCD_OK;
    }
    LQCHK(links_flush_of(c));
    return link_op<2>(C, mu_c, A, mu_a, B, mu_b, 0.0);
}
// mul!(C, A', B) on link fields (standardMD.jl:211: mul!(md.dSdU[mu], Uout[mu]', UdSfdUmu[mu])): C[mu_c](n) = A[mu_a](n)^+ B[mu_b](n)
extern "C" int lqcd_link_mul_adj(lqcd_gauge_t C, int mu_c, lqcd_gauge_t A, int mu_a, lqcd_gauge_t B, int mu_b) {
    LQCHK(link_args(C, mu_c, A, mu_a, "lqcd_link_mul_adj"));
    LQCHK(link_args(C, mu_c, B, mu_b, "lqcd_link_mul_adj"));
    LQCHK(links_flush_of(C));
    return link_op<6>(C, mu_c, A, mu_a, B, mu_b, 0.0);
}
// Traceless_antihermitian_add!(p[mu], factor, temp1) (AbstractMD.jl:110,131): P[mu_p] += factor * TA(G[mu_g]).  Third call of the P_update! triple:
// p[mu] += factor TA(U[mu] (beta/2) staples) in one pass
extern "C" int lqcd_link_add_ta(lqcd_gauge_t P, int mu_p, double factor, lqcd_gauge_t G, int mu_g) {
    LQCHK(link_args(P, mu_p, G, mu_g, "lqcd_link_add_ta"));
    ARGCHK(!(P == G && mu_p == mu_g), "lqcd_link_add_ta: P and G are the same link field");
    lqcd_ctx_s* c = P->ctx;
    LazyLinks& z = c->lazy;
    if (z.kind == 4 && z.T.is(G, mu_g) && P != z.Ug && P != z.T.g && P != z.S.g) {
        const LazyLinks r = z;
        z.kind = 0;
        if (mu_p == r.mu) {
            LazyLinks::Done d = {2, P, mu_p, factor, r.Ug, r.beta};
            return lazy_defer(c, d);
        }
        if (c->lazy.has_pend || c->lazy.has_pp) LQCHK(lazy_run_done(c));
        return staple_force(P, r.Ug, r.beta, factor, true, r.mu, mu_p, 0.5 * r.beta);
    }
    LQCHK(links_flush_of(c));
    return link_op<3>(P, mu_p, G, mu_g, nullptr, 0, factor);
}
// calc_dSdUmu!(dSdUmu, gauge_action, mu, U) (AbstractMD.jl:108) for the plaquette action pushed with coefficient beta/2
// (universe.jl:92-95): out[mu_out](n) = (beta/2) * sum of the six staples of U_mu(n), so that U_mu(n) out(n) is the plaquette
// sum whose -1/NC-weighted traceless anti-Hermitian part P_update! adds to p[mu].  Collective on a partitioned lattice.  First call of the
// P_update! triple: recorded
extern "C" int lqcd_link_staple(lqcd_gauge_t out, int mu_out, lqcd_gauge_t U, int mu, double beta) {
    LQCHK(link_args(out, mu_out, U, mu, "lqcd_link_staple"));
    ARGCHK(out != U, "lqcd_link_staple: out must not be the link field itself");
    lqcd_ctx_s* c = out->ctx;
    if (lazy_on(c)) {
        LQCHK(lazy_open_triple(c, 2, out));
        LazyLinks& z = c->lazy;
        z.kind = 3; z.S = lref(out, mu_out); z.Ug = U; z.mu = mu; z.beta = beta;
        return LQCD_OK;
    }
    LQCHK(links_flush_of(c));
    return staple_force(out, U, beta, 0.0, false, mu, mu_out, 0.5 * beta);
}

extern "C" int lqcd_link_exp_mul(lqcd_gauge_t W, int mu_w, double t, lqcd_gauge_t P, int mu_p, lqcd_gauge_t U, int mu_u) {
    LQCHK(link_args(W, mu_w, P, mu_p, "lqcd_link_exp_mul"));
    LQCHK(link_args(W, mu_w, U, mu_u, "lqcd_link_exp_mul"));
    ARGCHK(W != P && U != P, "lqcd_link_exp_mul: the momentum field must be a field of its own");
    LQCHK(links_flush_of(W));
    return link_exp_mul_now(W, mu_w, t, P, mu_p, U, mu_u);
}

// The three per-direction calls of the reference's P_update! (AbstractMD.jl:108-110) -- calc_dSdUmu!(dSdUmu, gauge_action, mu, U);
// mul!(temp1, U[mu], dSdUmu); Traceless_antihermitian_add!(p[mu], factor, temp1) -- as ONE pass: P[mu_p] += factor * TA(U[mu] * (beta/2) * staples);
// reached by the lazy triples above, or directly
extern "C" int lqcd_link_add_ta_staple(lqcd_gauge_t P, int mu_p, double factor, lqcd_gauge_t U, int mu, double beta) {
    LQCHK(link_args(P, mu_p, U, mu, "lqcd_link_add_ta_staple"));
    ARGCHK(P != U, "lqcd_link_add_ta_staple: the momentum field must not be the link field itself");
    LQCHK(links_flush_of(P));
    return staple_force(P, U, beta, factor, true, mu, mu_p, 0.5 * beta);
}

// P_update!(U, p, eps, md) (AbstractMD.jl:99-118) in one pass:  P += factor * TA(-(beta/6) U * staples); the force field is never stored
extern "C" int lqcd_momentum_add_gauge_force(lqcd_gauge_t P, double factor, lqcd_gauge_t U, double beta) {
    LQCHK(same_ctx(P, U, "lqcd_momentum_add_gauge_force"));
    lqcd_ctx_s* c = P->ctx;
    if (lazy_on(c) && c->tun.lazy_merge > 1) {      // waits for the link update that follows it (lazy_full_pupdate)
        LQCHK(links_flush(c));
        return lazy_full_pupdate(c, P, factor, U, beta);
    }
    LQCHK(links_flush_of(P));      // recorded single-direction link operations run first
    return staple_force(P, U, beta, factor, true);
}

// U_update! (AbstractMD.jl:78-97): U <- exp(dt P) U
extern "C" int lqcd_gauge_exp_update(lqcd_gauge_t U, double dt, lqcd_gauge_t P) {
    LQCHK(same_ctx(U, P, "lqcd_gauge_exp_update"));
    lqcd_ctx_s* c = U->ctx;
    if (lazy_on(c) && c->tun.lazy_merge && U != P) {      // waits for a second update of the same fields to merge with (lazy_full_update)
        const LazyLinks& z = c->lazy;
        if (z.kind || !z.done.empty()) LQCHK(links_flush(c));
        return lazy_full_update(c, U, dt, P);
    }
    LQCHK(links_flush_of(U));
    return gauge_exp_update_now(U, dt, P);
}
