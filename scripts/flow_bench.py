"""Gradient flow at 32^3x64 (hot start, thermalised by a few flow steps): one fused RK3 step (lqcd_gradient_flow), the same step composed from the MD
exports (lqcd_link_scaled_copy + lqcd_momentum_add_gauge_force at beta = 6 + lqcd_gauge_exp_update), one observables measurement, the resident
schedule (lqcd_gradient_flow_measure), and the MD block U_update! P_update! U_update! whose one-sweep kernel (gauge_force_kernel_tile<1, true>) is the
yardstick of a flow stage.  Wall times per call here; the kernel times come from running it under rocprofv3 --kernel-trace --stats.
usage: flow_bench.py [reps]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import latticeqcd_jl_amd as lq  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
L = (32, 32, 32, 64)
EPS = 0.01
f = lq.lib.lib()
U = lq.Initialize_Gaugefields(3, 0, *L, condition="hot", randomseed=111)
lat = U.lattice
lq.flow_(U, lq.Gradientflow(U, Nflow=3, eps=EPS))


def timed(fn, n):
    fn()
    lat.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    lat.sync()
    return 1e3 * (time.perf_counter() - t0) / n


fused = timed(lambda: lq.check(f.lqcd_gradient_flow(U._h, C.c_double(EPS), 1)), reps)

W = lq.Gaugefields(lat)
lq.substitute_U_(W, U)
X = lq.Gaugefields(lat)


def composed():
    for a, c in ((0.0, 0.25), (-17.0 / 9.0, 8.0 / 9.0), (-1.0, 0.75)):
        for mu in range(4):
            lq.check(f.lqcd_link_scaled_copy(X._h, mu, C.c_double(a), X._h, mu))
        lq.check(f.lqcd_momentum_add_gauge_force(X._h, C.c_double(c * EPS), W._h, C.c_double(6.0)))
        lq.check(f.lqcd_gauge_exp_update(W._h, C.c_double(1.0), X._h))


comp = timed(composed, reps)
W.close()
X.close()
obs = timed(lambda: lq.gauge_flow_observables(U), reps)
t0 = time.perf_counter()
tab = lq.gradient_flow_measure(U, EPS, 20, 5)
meas = 1e3 * (time.perf_counter() - t0)

p = lq.initialize_TA_Gaugefields(U)
lq.gauss_distribution_(p, 7)


def block():
    lq.U_update_(U, p, 0.5e-9)
    lq.P_update_(U, p, 1e-9, 5.7)
    lq.U_update_(U, p, 0.5e-9)


md = timed(block, reps)
V = L[0] * L[1] * L[2] * L[3]
print(f"lattice {L}  reps {reps}")
print(f"fused RK3 step (lqcd_gradient_flow, 1 step)        {fused:8.3f} ms wall")
print(f"composed RK3 step (MD exports)                     {comp:8.3f} ms wall   fused / composed = {fused / comp:.3f}")
print(f"observables (lqcd_gauge_flow_observables)          {obs:8.3f} ms wall")
print(f"resident schedule, 20 steps + 4 measurements       {meas:8.3f} ms wall   ({meas / 20:.3f} ms per step incl. measurements)")
print(f"MD block U_update! P_update! U_update!             {md:8.3f} ms wall")
print(f"compulsory bytes of the observables launch: {V * 4 * 144 / 1e9:.3f} GB (the links once)")
print("last table row:", " ".join(f"{v:.10g}" for v in tab[-1]))
