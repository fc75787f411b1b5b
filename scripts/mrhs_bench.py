"""Several right-hand sides at 32^3x64, kappa = 0.12 (hot start, smoothed by three flow steps -- the configuration of profiles/r12_meson.log): wall times of
  a. one lqcd_op_hop_multi with n = 2, 3, 4 columns against n lqcd_op_hop calls (the single-column kernel, unchanged) -- model: 0.50 of four single hops at n = 4,
  b. lqcd_solve_bicgstab_eo_multi on the four spin columns of one source colour against four lqcd_solve_bicgstab_eo calls with the default bicg_fused:
     wall time and time per column iteration -- model: 0.70 per iteration,
  c. lqcd_meson_correlators with meson_mrhs = 1 against the same call with meson_mrhs = 0.
Three rounds in alternation; the sub-millisecond calls are timed over windows of 300 calls.  Every ratio is reported with its spread over the rounds.
usage: mrhs_bench.py [log file, default profiles/r14_mrhs.log] [solver reps per round, default 5]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import latticeqcd_jl_amd as lq  # noqa: E402

log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14_mrhs.log")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
WINDOW, ROUNDS = 300, 3
L = (32, 32, 32, 64)
KAPPA = 0.12
log = open(log_path, "w")


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


U = lq.Initialize_Gaugefields(3, 0, *L, condition="hot", randomseed=111)
lat = U.lattice
lq.flow_(U, lq.Gradientflow(U, Nflow=3, eps=0.01))
D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "r": 1.0, "eps_CG": 1e-19, "MaxCGstep": 3000, "method_CG": "bicgstab_evenodd"})
src = (0, 0, 0, 0)


def timed(fn, n):
    fn()
    lat.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    lat.sync()
    return 1e3 * (time.perf_counter() - t0) / n


def ratio_line(what, new, old):
    r = [a / b for a, b in zip(new, old)]
    return f"{what}: {np.median(new):9.4f} ms against {np.median(old):9.4f} ms   ratio {np.median(r):.3f} (rounds {min(r):.3f} .. {max(r):.3f})"


say(f"lattice {L}  kappa {KAPPA}  plaquette {lq.calculate_Plaquette(U):.6f}  windows of {WINDOW} calls, {ROUNDS} rounds in alternation, medians")

# ---------------------------------------------------------------- a. the hop
xs = [lq.Fermionfields(lat, lq.WILSON, lq.ODD) for _ in range(4)]
ys = [lq.Fermionfields(lat, lq.WILSON, lq.EVEN) for _ in range(4)]
for j, x in enumerate(xs):
    lq.gauss_distribution_fermion_(x, 500 + j)
lq.hop_multi_(ys, D, xs)
say(f"a. parity hop (even output), 12-real links: recon_active {lat.get_param('recon_active')}, mrhs_active {lat.get_param('mrhs_active')}")
one = []
res = {n: ([], []) for n in (2, 3, 4)}
for _ in range(ROUNDS):
    one.append(timed(lambda: lq.hop_(ys[0], D, xs[0]), WINDOW))
    for n in (2, 3, 4):
        res[n][1].append(timed(lambda: [lq.hop_(ys[j], D, xs[j]) for j in range(n)], WINDOW))
        res[n][0].append(timed(lambda: lq.hop_multi_(ys[:n], D, xs[:n]), WINDOW))
say(f"   one lqcd_op_hop call (with its host synchronisation): {np.median(one):.4f} ms")
for n in (2, 3, 4):
    say("   " + ratio_line(f"lqcd_op_hop_multi n = {n} against {n} lqcd_op_hop calls", res[n][0], res[n][1]))
model = {2: (768 / 2 + 384) / 1152, 3: (768 / 3 + 384) / 1152, 4: (768 / 4 + 384) / 1152}
say("   byte model (768 / n + 384) / 1152: " + "  ".join(f"n = {n}: {model[n]:.2f}" for n in (2, 3, 4)))
del xs, ys

# ---------------------------------------------------------------- b. the solver
bs = [lq.Fermionfields(lat, lq.WILSON) for _ in range(4)]
sol = [lq.Fermionfields(lat, lq.WILSON) for _ in range(4)]
for isp, b in enumerate(bs):
    lq.setindex_global_(b, 0, *src, isp)
its_s, its_m = [0] * 4, [0] * 4


def single():
    for j in range(4):
        lq.clear_fermion_(sol[j])
        its_s[j] = lq.solve_DinvX_(sol[j], D, bs[j], return_info=True)[0]


def multi():
    for j in range(4):
        lq.clear_fermion_(sol[j])
    its_m[:] = lq.solve_DinvX_multi_(sol, D, bs, return_info=True)[0]


ts, tm = [], []
for _ in range(ROUNDS):
    ts.append(timed(single, reps))
    tm.append(timed(multi, reps))
say(f"b. four spin columns of source colour 0, eps 1e-19: iterations single {its_s} (bicg_fused {lat.get_param('bicg_fused')}), multi {its_m} (mrhs_active {lat.get_param('mrhs_active')})")
say("   " + ratio_line("lqcd_solve_bicgstab_eo_multi against four lqcd_solve_bicgstab_eo calls, wall", tm, ts))
say("   " + ratio_line("the same per column iteration", [t / sum(its_m) for t in tm], [t / sum(its_s) for t in ts]) + "   model 0.70")

# ---------------------------------------------------------------- c. the meson table
t0s, t1s = [], []
for _ in range(ROUNDS):
    lat.set_param("meson_mrhs", 0)
    t0s.append(timed(lambda: lq.meson_correlators(D, src), max(1, reps // 2)))
    lat.set_param("meson_mrhs", 1)
    t1s.append(timed(lambda: lq.meson_correlators(D, src), max(1, reps // 2)))
tab1 = lq.meson_correlators(D, src)
lat.set_param("meson_mrhs", 0)
tab0 = lq.meson_correlators(D, src)
say("c. " + ratio_line("lqcd_meson_correlators with meson_mrhs = 1 against meson_mrhs = 0", t1s, t0s) + "   (profiles/r12_meson.log: 157.8 ms)")
say("   max |C(meson_mrhs = 1) - C(0)| / C_15 =", float((np.abs(tab1 - tab0) / tab0[15]).max()))
