"""Quenched heatbath at 32^3x64 (cold start, thermalised by heatbath + OR updates at beta = 6): one heatbath sweep (lqcd_gauge_heatbath, 8 launches),
one OR sweep (lqcd_gauge_overrelax), the resident schedule (lqcd_gauge_heatbath_measure) per sweep, and the staple-force sweep (lqcd_gauge_force) that
is the yardstick of both.  The rejection trials per SU(2) draw come from the numpy restatement (tests/heatbath_numpy.py) run over every link of one
sweep of a 6^4 configuration thermalised at the same beta on the device: the trials depend on beta and the ensemble, not on the volume.  At 12^4 the
wall time of one heatbath + 3 OR update is set beside one 33-step quenched HMC trajectory of tests/test_gpu_quenched_literature.py.  Wall times per
call here; the kernel times come from running it under rocprofv3 --kernel-trace --stats.
usage: heatbath_bench.py [reps]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import latticeqcd_jl_amd as lq  # noqa: E402
import heatbath_numpy as hn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
BETA = 6.0
f = lq.lib.lib()


def timed(lat, fn, n):
    fn()
    lat.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    lat.sync()
    return 1e3 * (time.perf_counter() - t0) / n


L = (32, 32, 32, 64)
U = lq.Initialize_Gaugefields(3, 0, *L, condition="cold")
lat = U.lattice
hb = lq.Heatbath(U, BETA, seed=1)
therm = lq.heatbath_measure(U, hb, 20, numOR=3)
hbs = timed(lat, lambda: lq.heatbath_(U, hb), reps)
ors = timed(lat, lambda: lq.overrelaxation_(U, hb), reps)
t0 = time.perf_counter()
tab = lq.heatbath_measure(U, hb, reps)
meas = 1e3 * (time.perf_counter() - t0) / reps
G = lq.Gaugefields(lat)
force = timed(lat, lambda: lq.check(f.lqcd_gauge_force(G._h, U._h, C.c_double(BETA))), reps)
G.close()
V = L[0] * L[1] * L[2] * L[3]
# compulsory traffic of a sweep: each of the 8 (mu, parity) launches reads the whole field once (the other directions at both parities, U_mu at the
# other one) and writes its half of U_mu: 8 x 4V x 144 + 4V x 144 B = 9 x 144 B per link
bytes_sweep = 9 * 144 * 4 * V
print(f"lattice {L}  beta {BETA}  reps {reps}  plaquette after thermalisation {therm[-1]:.6f}, after the runs {tab[-1]:.6f}")
print(f"heatbath sweep (lqcd_gauge_heatbath, 1 sweep)      {hbs:8.3f} ms wall   / staple-force sweep = {hbs / force:.2f} (target <= 2)")
print(f"OR sweep (lqcd_gauge_overrelax, 1 sweep)           {ors:8.3f} ms wall   / staple-force sweep = {ors / force:.2f} (target <= 1.5)")
print(f"heatbath_measure, per sweep (sweep + plaquette)    {meas:8.3f} ms wall")
print(f"staple-force sweep (lqcd_gauge_force)              {force:8.3f} ms wall")
print(f"compulsory bytes per sweep: {bytes_sweep / 1e9:.3f} GB ({9 * 144} B per link); at the heatbath sweep's wall time "
      f"{bytes_sweep / (hbs * 1e-3) / 1e12:.2f} TB/s = {100 * bytes_sweep / (hbs * 1e-3) / 8e12:.1f} % of 8 TB/s, OR sweep "
      f"{100 * bytes_sweep / (ors * 1e-3) / 8e12:.1f} %")
U.close()

# rejection trials per SU(2) draw, from the restatement on an equilibrium 6^4 configuration at the same beta
L6 = (6, 6, 6, 6)
U6 = lq.Initialize_Gaugefields(3, 0, *L6, condition="cold")
lq.heatbath_measure(U6, lq.Heatbath(U6, BETA, seed=2), 100, numOR=3)
counts = {}
hn.sweep(U6.download(), L6, False, BETA, 10**5, 3, 0, counts)
for b in ("kp", "creutz", "haar"):
    if counts.get(b):
        print(f"trials per draw ({b:6s}): mean {counts[b + '_trials'] / counts[b]:.4f}, max {counts[b + '_max']}  over {counts[b]} draws "
              f"(restatement, one sweep of 6^4 at beta {BETA})")

# 12^4: one heatbath + 3 OR update against one 33-step quenched HMC trajectory (tests/test_gpu_quenched_literature.py::_run)
L12 = (12, 12, 12, 12)
U = lq.Initialize_Gaugefields(3, 0, *L12, condition="cold")
lat = U.lattice
m = lq.Heatbathupdate(U, None, True, useOR=True, numOR=3, beta=5.7)
for _ in range(20):
    lq.update_(m, U)
upd = timed(lat, lambda: lq.update_(m, U), reps)
p, Uold = lq.initialize_TA_Gaugefields(U), lq.Gaugefields(lat)
rng = np.random.default_rng(5)


def trajectory(beta=5.7, dtau=0.03, mdsteps=33):
    lq.substitute_U_(Uold, U)
    lq.gauss_distribution_(p, int(rng.integers(1 << 30)))
    H0 = lq.momentum_action(p) + lq.evaluate_GaugeAction(U, beta)
    for _ in range(mdsteps):
        lq.U_update_(U, p, 0.5 * dtau)
        lq.P_update_(U, p, dtau, beta)
        lq.U_update_(U, p, 0.5 * dtau)
    dH = lq.momentum_action(p) + lq.evaluate_GaugeAction(U, beta) - H0
    if not (dH <= 0 or np.exp(-dH) >= rng.random()):
        lq.substitute_U_(U, Uold)


traj = timed(lat, trajectory, reps)
print(f"12^4 beta 5.7: heatbath + 3 OR update (update_) {upd:8.3f} ms wall;  one 33-step quenched HMC trajectory {traj:8.3f} ms wall  "
      f"(ratio {traj / upd:.1f})")
