// bench_api.hip -- timing entry points (HIP events on the library's own stream) and the externally timed CG session used by bench.py.
#include "ops_internal.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <functional>

using namespace lqcd;

// ---------------------------------------------------------------------------------- C API: timing
extern "C" int lqcd_bench_dslash(lqcd_op_t op, lqcd_spinor_t out, lqcd_spinor_t in, int dagger, int warm, int reps, double* ms) {
    LQCHK(check_full(op, out, in, "lqcd_bench_dslash"));
    ARGCHK(reps > 0 && ms, "lqcd_bench_dslash: bad reps");
    lqcd_ctx_s* c = op->ctx;
    HIPCHK(hipSetDevice(c->device));
    for (int i = 0; i < warm; i++) LQCHK(op_apply_async(op, out, in, dagger ? 1 : 0, nullptr));
    HIPCHK(hipEventRecord(c->ev_t0, c->stream));
    for (int i = 0; i < reps; i++) LQCHK(op_apply_async(op, out, in, dagger ? 1 : 0, nullptr));
    HIPCHK(hipEventRecord(c->ev_t1, c->stream));
    HIPCHK(hipEventSynchronize(c->ev_t1));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, c->ev_t0, c->ev_t1));
    *ms = (double)t / reps;
    return LQCD_OK;
}

// SURVEY.md 8(d) timing protocol: every application bracketed by its own HIP events, median (and mean) over `reps`
extern "C" int lqcd_bench_dslash_median(lqcd_op_t op, lqcd_spinor_t out, lqcd_spinor_t in, int dagger, int warm, int reps, double* median_ms,
                                        double* mean_ms) {
    LQCHK(check_full(op, out, in, "lqcd_bench_dslash_median"));
    ARGCHK(reps > 0 && reps <= 4096 && median_ms, "lqcd_bench_dslash_median: bad reps");
    lqcd_ctx_s* c = op->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::vector<hipEvent_t> ev(reps + 1);
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    for (int i = 0; i < warm; i++) LQCHK(op_apply_async(op, out, in, dagger ? 1 : 0, nullptr));
    HIPCHK(hipEventRecord(ev[0], c->stream));
    for (int i = 0; i < reps; i++) {
        LQCHK(op_apply_async(op, out, in, dagger ? 1 : 0, nullptr));
        HIPCHK(hipEventRecord(ev[i + 1], c->stream));
    }
    HIPCHK(hipEventSynchronize(ev[reps]));
    std::vector<double> t(reps);
    double sum = 0;
    for (int i = 0; i < reps; i++) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        t[i] = ms;
        sum += ms;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    std::sort(t.begin(), t.end());
    *median_ms = reps % 2 ? t[reps / 2] : 0.5 * (t[reps / 2 - 1] + t[reps / 2]);
    if (mean_ms) *mean_ms = sum / reps;
    return LQCD_OK;
}

// Phase breakdown of ONE partitioned operator application (mean over reps, each rep synchronised):
//   ms[0] pack, ms[1] interior kernel (overlapping the exchange), ms[2] exchange = pack end -> last halo byte received (RCCL on the
//   communication stream, incl. its launch latency), ms[3] compute stream idle waiting for the exchange after the interior,
//   ms[4] exterior, ms[5] whole application.  What the N > 1 lines of bench.py report, so that the critical path of the halo
//   exchange on real xGMI links is visible from the driver's multi-GPU runs.
extern "C" int lqcd_bench_halo_phases(lqcd_op_t op, lqcd_spinor_t out, lqcd_spinor_t in, int dagger, int reps, double* ms) {
    LQCHK(check_full(op, out, in, "lqcd_bench_halo_phases"));
    ARGCHK(reps > 0 && ms, "lqcd_bench_halo_phases: bad arguments");
    lqcd_ctx_s* c = op->ctx;
    ARGCHK(any_partitioned(c) && c->has_comm && c->local_peers.empty(), "lqcd_bench_halo_phases: needs a partitioned context with a communicator (RCCL or peer-mapped)");
    HIPCHK(hipSetDevice(c->device));
    hipEvent_t e[6];
    for (auto& ev : e) HIPCHK(hipEventCreate(&ev));
    double acc[6] = {0, 0, 0, 0, 0, 0};
    apply_bc(c, op->bc);
    StencilCall s;
    LQCHK(make_full_call(op, out, in, dagger ? 1 : 0, s));
    LQCHK(halo_schedule_settle(op));
    // the folded one-stream schedule (round 5; what the solvers run when the collective timing picked schedule 3 and halo_fold applies): pack -> exchange ->
    // ONE stencil launch that takes the boundary hops from the ghost buffers.  ms[1] = that launch, ms[2] = the exchange, ms[3] = ms[4] = 0: nothing waits and
    // there is no exterior kernel.  (Inside the fused CG the pack launch is gone as well: the x/p update and the reduction launch write the faces.)
    if (halo_fold_applies(c, s.kind, s.r, s.parity_mode, s.prec, s.clover != nullptr)) {
        StencilCall f = s;
        f.fold = 1;
        for (int r = 0; r < reps + 2; r++) {
            HIPCHK(hipEventRecord(e[0], c->stream));
            LQCHK(launch_stencil_pack(c, s));
            HIPCHK(hipEventRecord(e[1], c->stream));
            LQCHK(comm_halo_exchange(c, s.kind, s.parity_mode, 0, 1));
            HIPCHK(hipEventRecord(e[2], c->stream));
            LQCHK(launch_stencil_interior(c, f));
            HIPCHK(hipEventRecord(e[3], c->stream));
            HIPCHK(hipEventSynchronize(e[3]));
            if (r < 2) continue;
            float t;
            HIPCHK(hipEventElapsedTime(&t, e[0], e[1])); acc[0] += t;
            HIPCHK(hipEventElapsedTime(&t, e[1], e[2])); acc[2] += t;
            HIPCHK(hipEventElapsedTime(&t, e[2], e[3])); acc[1] += t;
            HIPCHK(hipEventElapsedTime(&t, e[0], e[3])); acc[5] += t;
        }
        for (int k = 0; k < 6; k++) ms[k] = acc[k] / reps;
        for (auto& ev : e) (void)hipEventDestroy(ev);
        return LQCD_OK;
    }
    for (int r = 0; r < reps + 2; r++) {          // two untimed warm-up applications
        HIPCHK(hipEventRecord(e[0], c->stream));
        LQCHK(launch_stencil_pack(c, s));
        HIPCHK(hipEventRecord(e[1], c->stream));
        LQCHK(comm_halo_exchange(c, s.kind, s.parity_mode, 0, 0));
        HIPCHK(hipEventRecord(e[5], c->comm_stream));
        LQCHK(launch_stencil_interior(c, s));
        HIPCHK(hipEventRecord(e[2], c->stream));
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_comm, 0));
        HIPCHK(hipEventRecord(e[3], c->stream));
        LQCHK(launch_stencil_exterior(c, s));
        HIPCHK(hipEventRecord(e[4], c->stream));
        HIPCHK(hipEventSynchronize(e[4]));
        HIPCHK(hipEventSynchronize(e[5]));
        if (r < 2) continue;
        float t;
        HIPCHK(hipEventElapsedTime(&t, e[0], e[1])); acc[0] += t;
        HIPCHK(hipEventElapsedTime(&t, e[1], e[2])); acc[1] += t;
        HIPCHK(hipEventElapsedTime(&t, e[1], e[5])); acc[2] += t;
        HIPCHK(hipEventElapsedTime(&t, e[2], e[3])); acc[3] += t;
        HIPCHK(hipEventElapsedTime(&t, e[3], e[4])); acc[4] += t;
        HIPCHK(hipEventElapsedTime(&t, e[0], e[4])); acc[5] += t;
    }
    for (int k = 0; k < 6; k++) ms[k] = acc[k] / reps;
    for (auto& ev : e) (void)hipEventDestroy(ev);
    return LQCD_OK;
}

// mean latency (microseconds) of the stream-ordered one-double all-reduce the solvers issue twice per CG iteration
extern "C" int lqcd_bench_allreduce(lqcd_ctx_t c, int reps, double* us) {
    ARGCHK(c && reps > 0 && us, "lqcd_bench_allreduce: bad arguments");
    ARGCHK(c->has_comm, "lqcd_bench_allreduce: communicators not initialised");
    HIPCHK(hipSetDevice(c->device));
    double* d = c->d_scal + S_RED0;
    HIPCHK(hipMemsetAsync(d, 0, sizeof(double), c->stream));   // 0 + 0 + ... stays finite however often it is summed
    for (int i = 0; i < 5; i++) LQCHK(comm_allreduce(c, d, 1));
    HIPCHK(hipEventRecord(c->ev_t0, c->stream));
    for (int i = 0; i < reps; i++) LQCHK(comm_allreduce(c, d, 1));
    HIPCHK(hipEventRecord(c->ev_t1, c->stream));
    HIPCHK(hipEventSynchronize(c->ev_t1));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, c->ev_t0, c->ev_t1));
    *us = 1e3 * (double)t / reps;
    return LQCD_OK;
}

extern "C" int lqcd_bench_cg(lqcd_op_t op, lqcd_spinor_t x, lqcd_spinor_t b, int warm, int niter, double* ms_per_iter) {
    LQCHK(check_full(op, x, b, "lqcd_bench_cg"));
    ARGCHK(niter > 0 && ms_per_iter, "lqcd_bench_cg: bad niter");
    lqcd_ctx_s* c = op->ctx;
    HIPCHK(hipSetDevice(c->device));
    CgWork w;
    LQCHK(cg_work_get(c, x->kind, w));
    double rr;
    int st = cg_setup(op, x, b, w, -1.0, &rr);
    for (int i = 0; i < warm && st == LQCD_OK; i++) st = cg_enqueue_iteration(op, x, w);
    if (st == LQCD_OK) {
        (void)hipEventRecord(c->ev_t0, c->stream);
        for (int i = 0; i < niter && st == LQCD_OK; i++) st = cg_enqueue_iteration(op, x, w);
        (void)hipEventRecord(c->ev_t1, c->stream);
        hipError_t e = hipEventSynchronize(c->ev_t1);
        float t = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, c->ev_t0, c->ev_t1);
        if (e != hipSuccess && st == LQCD_OK) st = hip_fail(e, "bench_cg timing", __FILE__, __LINE__);
        *ms_per_iter = (double)t / niter;
    }
    { const int fs = cg_finish(op, x, w, st == LQCD_OK); if (st == LQCD_OK) st = fs; }
    (void)hipStreamSynchronize(c->stream);
    cg_work_put(w);
    return st;
}

// one launch of a full-lattice stencil with the epilogues the fused CG uses, on caller-owned fields (tests): mode 0 plain, dst = D in; 1 update mode, dst = src - coef D in
// (src may be dst: the in-place launch); 2 recurrence mode, dst = D in + coef dst.  D^+ with dagger, the temporal-gauge copy of the links with tgauge (8: its 8-real form), `done` is written to
// the done flag first (modes 1 and 2 are then no-ops) and cleared afterwards.  norm2: the sum of the launch's |.|^2 partials.
extern "C" int lqcd_bench_stencil_epilogue(lqcd_op_t op, lqcd_spinor_t dst, lqcd_spinor_t src, lqcd_spinor_t in, int dagger, int mode, int tgauge, double coef, int done, double* norm2) {
    LQCHK(check_full(op, dst, in, "lqcd_bench_stencil_epilogue"));
    ARGCHK(mode >= 0 && mode <= 2 && norm2 && (mode != 1 || src), "lqcd_bench_stencil_epilogue: bad arguments");
    if (mode == 1) LQCHK(check_full(op, src, in, "lqcd_bench_stencil_epilogue"));
    ARGCHK(in != dst && in != src, "lqcd_bench_stencil_epilogue: the hop operand must not be written");
    lqcd_ctx_s* c = op->ctx;
    HIPCHK(hipSetDevice(c->device));
    const double2 *gt = nullptr, *gt8 = nullptr;
    if (tgauge) {
        ARGCHK(gauge_ensure_tgauge(op->gauge) == LQCD_OK && op->gauge->tgauge_ok, "lqcd_bench_stencil_epilogue: no temporal-gauge copy of these links");
        gt = op->gauge->data12t;
        if (tgauge == 8) {      // ... in its 8-real form
            ARGCHK(gauge_ensure_tgauge(op->gauge, true) == LQCD_OK && op->gauge->data8t && op->gauge->tgauge8_dev <= 1e-14, "lqcd_bench_stencil_epilogue: no 8-real temporal-gauge copy of these links");
            gt8 = op->gauge->data8t;
        }
    }
    double sc[3] = {coef, coef, done ? 1.0 : 0.0};      // S_ALPHA, S_BETA, S_DONE
    static_assert(S_BETA == S_ALPHA + 1 && S_DONE == S_ALPHA + 2, "lqcd_bench_stencil_epilogue: scalar slots");
    HIPCHK(hipMemcpyAsync(c->d_scal + S_ALPHA, sc, sizeof(sc), hipMemcpyHostToDevice, c->stream));
    apply_bc(c, op->bc);
    StencilCall s;
    LQCHK(make_full_call(op, dst, in, dagger, s));
    s.gauge12t = gt;
    s.gauge8t = gt8;
    s.norm_partial = c->d_partial;
    if (mode) {
        s.upd_scal = c->d_scal;
        for (int q = 0; q < 2; q++) { s.upd[q] = spinor_block(dst, q); if (mode == 1 && src != dst) s.upd_src[q] = spinor_block(src, q); }
        s.upd_rec = mode == 2 ? 1 : 0;
    }
    int st = stencil_apply(c, s);
    if (st == LQCD_OK) st = reduce_to_slot(c, stencil_num_partials(c, op->kind, op->r, 2, 0, op_fused_clover(op)), 1, S_PQ, true);
    sc[2] = 0.0;
    HIPCHK(hipMemcpyAsync(c->d_scal + S_ALPHA, sc, sizeof(sc), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_scal, c->d_scal + S_PQ, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *norm2 = c->h_scal[0];
    return st;
}

// the same for the fp32 build and the site-pair kernel: one launch of the stencil a mixed-precision solve on `op` would run (links, layout and kernel from mix_prepare),
// with the epilogues of inner_cg32 (modes 0, 1) or one schur32 application of the mixed even-odd BiCGStab (mode 2, even halves of FULL fields) -- mixed.hip
extern "C" int lqcd_bench_stencil_f32(lqcd_op_t op, lqcd_spinor_t dst, lqcd_spinor_t src, lqcd_spinor_t in, lqcd_spinor_t z, lqcd_spinor_t z2, int dagger, int mode,
                                      double coef, int done, int conj, int soa, double* sums) {
    LQCHK(check_full(op, dst, in, "lqcd_bench_stencil_f32"));
    ARGCHK(mode >= 0 && mode <= 2 && sums && (mode != 1 || src) && (mode != 2 || z), "lqcd_bench_stencil_f32: bad arguments");
    if (mode == 1) LQCHK(check_full(op, src, in, "lqcd_bench_stencil_f32"));
    if (mode == 2) LQCHK(check_full(op, z, dst, "lqcd_bench_stencil_f32"));
    if (mode == 2 && z2) LQCHK(check_full(op, z2, in, "lqcd_bench_stencil_f32"));
    ARGCHK(mode != 2 || !z2 || z == in, "lqcd_bench_stencil_f32: the second inner product exists for z = in only (the <s, t>, |t|^2, <r0, t> launch of the merged chain)");
    ARGCHK(in != dst, "lqcd_bench_stencil_f32: the hop operand must not be written");
    HIPCHK(hipSetDevice(op->ctx->device));
    return mixed_bench_stencil_f32(op, dst, src, in, z, z2, dagger, mode, coef, done, conj, soa, sums);
}

// the one-block final reduction (blas.hip reduce_final behind reduce_to_slot, single rank, no scalar step) on partials the caller supplies (tests): a device buffer of
// its own holds them (d_partial is too small for the large counts) with 64 NaNs behind them, so a read past the last partial poisons its sum instead of leaving the
// buffer; out = d_scal[S_RED0 .. S_RED0 + nvals).  guard = the two slots behind the sums, which the call must not write: they are set to LQCD_BENCH_REDUCE_SENTINEL
// before the launch, read back after it and then restored.
extern "C" int lqcd_bench_reduce_partials(lqcd_ctx_t c, const double* host_partials, int nblocks, int nvals, int soa, double* out, double* guard) {
    ARGCHK(c && host_partials && out && guard, "lqcd_bench_reduce_partials: null argument");
    ARGCHK(nvals >= 1 && nvals <= PEER_RED_VALS && nblocks >= 1, "lqcd_bench_reduce_partials: one to eight values per block, at least one block");
    static_assert(S_RED0 + PEER_RED_VALS + 2 <= SCAL_DOUBLES, "lqcd_bench_reduce_partials: guard slots");
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)nblocks * nvals;
    double* buf = nullptr;
    constexpr int TAIL = 64;
    HIPCHK(hipMalloc((void**)&buf, (n + TAIL) * sizeof(double)));
    double* const g = c->d_scal + S_RED0 + nvals;
    const double sentinel[2] = {LQCD_BENCH_REDUCE_SENTINEL, LQCD_BENCH_REDUCE_SENTINEL};
    double keep[2] = {0, 0}, res[PEER_RED_VALS + 2], tail[TAIL];
    for (double& t : tail) t = std::nan("");
    int st = LQCD_OK;
    auto hip = [&](hipError_t e, const char* what) { if (e != hipSuccess && st == LQCD_OK) st = hip_fail(e, what, __FILE__, __LINE__); return st == LQCD_OK; };
    bool armed = false;
    if (hip(hipMemcpyAsync(buf, host_partials, n * sizeof(double), hipMemcpyHostToDevice, c->stream), "H2D partials") &&
        hip(hipMemcpyAsync(buf + n, tail, sizeof tail, hipMemcpyHostToDevice, c->stream), "H2D tail") &&
        hip(hipMemcpyAsync(keep, g, sizeof keep, hipMemcpyDeviceToHost, c->stream), "D2H guard slots") && hip(hipStreamSynchronize(c->stream), "sync") &&
        hip(hipMemcpyAsync(g, sentinel, sizeof sentinel, hipMemcpyHostToDevice, c->stream), "H2D sentinel")) {
        armed = true;
        st = reduce_to_slot(c, nblocks, nvals, S_RED0, /*allreduce*/ false, 0, buf, soa != 0);
        if (st == LQCD_OK) hip(hipMemcpyAsync(res, c->d_scal + S_RED0, (nvals + 2) * sizeof(double), hipMemcpyDeviceToHost, c->stream), "D2H sums");
    }
    if (armed) {      // the slots get their values back whatever happened in between
        const hipError_t e = hipMemcpyAsync(g, keep, sizeof keep, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess && st == LQCD_OK) st = hip_fail(e, "H2D guard slots", __FILE__, __LINE__);
    }
    { const hipError_t e = hipStreamSynchronize(c->stream); if (e != hipSuccess && st == LQCD_OK) st = hip_fail(e, "sync", __FILE__, __LINE__); }
    (void)hipFree(buf);
    if (st != LQCD_OK) return st;
    for (int v = 0; v < nvals; v++) out[v] = res[v];
    guard[0] = res[nvals];
    guard[1] = res[nvals + 1];
    return LQCD_OK;
}

// CG session (externally timed windows); the state lives in the context, one open session per context
namespace lqcd {
struct CgSession { lqcd_op_s* op = nullptr; lqcd_spinor_s* x = nullptr; CgWork w; };
}
extern "C" int lqcd_cg_session_begin(lqcd_op_t op, lqcd_spinor_t x, lqcd_spinor_t b) {
    LQCHK(check_full(op, x, b, "lqcd_cg_session_begin"));
    lqcd_ctx_s* c = op->ctx;
    ARGCHK(c->cg_session == nullptr, "lqcd_cg_session_begin: a session is already open on this context");
    HIPCHK(hipSetDevice(c->device));
    CgSession* ses = new CgSession;
    CgWork& w = ses->w;
    int st = cg_work_get(c, x->kind, w);
    double rr;
    if (st == LQCD_OK) st = cg_setup(op, x, b, w, -1.0, &rr);
    if (st != LQCD_OK) {
        (void)cg_finish(op, x, w, false);      // (a set-up that failed behind its rotation of x)
        cg_work_put(w);
        delete ses;
        return st;
    }
    ses->op = op;
    ses->x = x;
    c->cg_session = ses;
    return LQCD_OK;
}
extern "C" int lqcd_cg_session_iterate(lqcd_op_t op, int n) {
    LQCHK(lqcd::links_flush_of(op));      // recorded single-direction link operations run first (links.hip)
    ARGCHK(op && op->ctx->cg_session && static_cast<CgSession*>(op->ctx->cg_session)->op == op, "lqcd_cg_session_iterate: no open session for this operator");
    CgSession* ses = static_cast<CgSession*>(op->ctx->cg_session);
    if (cg_gauge_moved(op, ses->w)) {
        set_error("lqcd_cg_session_iterate: the gauge field changed under the open session (it iterates in the temporal gauge of the links it was begun on): end it and begin a new one");
        return LQCD_ERR_ARG;
    }
    for (int i = 0; i < n; i++) LQCHK(cg_enqueue_iteration(op, ses->x, ses->w));
    HIPCHK(hipStreamSynchronize(op->ctx->stream));
    return LQCD_OK;
}
extern "C" int lqcd_cg_session_end(lqcd_op_t op) {
    ARGCHK(op && op->ctx->cg_session && static_cast<CgSession*>(op->ctx->cg_session)->op == op, "lqcd_cg_session_end: no open session for this operator");
    CgSession* ses = static_cast<CgSession*>(op->ctx->cg_session);
    CgWork& w = ses->w;
    const int st = cg_finish(op, ses->x, w);       // a pending deferred x update (and x back from temporal gauge); its status is the status of the session
    (void)hipStreamSynchronize(op->ctx->stream);
    cg_work_put(w);
    delete ses;
    op->ctx->cg_session = nullptr;
    return st;
}
