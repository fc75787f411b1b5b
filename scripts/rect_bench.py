"""The plaquette + rectangle action at 32^3x64 (hot start, smoothed by three flow steps, every link projected onto the group so that the sweeps load two rows):
wall times of
  a. lqcd_momentum_add_gauge_force, the plaquette staple sweep -- the yardstick,
  b. lqcd_momentum_add_gauge_force_improved with Luscher-Weisz coefficients (operation count: 72 + 1 matrix products per link against 12 + 1, 96 + 1 link loads
     against 18 + 1; a ratio above 7 would be a defect), also with staple_recon = 0 (all 18 reals of every link),
  c. lqcd_gauge_plaquette against lqcd_gauge_rectangle.
Three rounds in alternation, windows of 300 calls, every call with its host synchronisation; lazy_links = 0, so that every call runs when it is made.
usage: rect_bench.py [log file, default profiles/r18_rect_action.log]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import latticeqcd_jl_amd as lq  # noqa: E402

log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r18_rect_action.log")
WINDOW, ROUNDS = 300, 3
L = (32, 32, 32, 64)
BETA = 5.7
BP, BR = 5.0 * BETA / 3.0, -BETA / 12.0
log = open(log_path, "w")


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


U = lq.Initialize_Gaugefields(3, 0, *L, condition="hot", randomseed=111)
lat = U.lattice
lat.set_param("lazy_links", 0)
lq.flow_(U, lq.Gradientflow(U, Nflow=3, eps=0.01))
lq.reunitarize_(U)
p = lq.initialize_TA_Gaugefields(U)
lq.gauss_distribution_(p, 7)


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


say(f"lattice {L}  beta {BETA}  Luscher-Weisz beta_plaq {BP:.4f} beta_rect {BR:.4f}  plaquette {lq.calculate_Plaquette(U):.6f}  rectangle {lq.calculate_Rectangle(U):.6f}")
say(f"windows of {WINDOW} calls, {ROUNDS} rounds in alternation, medians; factor 1e-6 (the momenta stay O(1))")
ta, tb, tb18, tp, tr = [], [], [], [], []
for _ in range(ROUNDS):
    ta.append(timed(lambda: lq.P_update_(U, p, 1e-6, BETA), WINDOW))
    tb.append(timed(lambda: lq.P_update_(U, p, 1e-6, BP, BR), WINDOW))
    lat.set_param("staple_recon", 0)
    tb18.append(timed(lambda: lq.P_update_(U, p, 1e-6, BP, BR), WINDOW))
    lat.set_param("staple_recon", 1)
    tp.append(timed(lambda: lq.calculate_Plaquette(U), WINDOW))
    tr.append(timed(lambda: lq.calculate_Rectangle(U), WINDOW))
say("a./b. " + ratio_line("lqcd_momentum_add_gauge_force_improved against lqcd_momentum_add_gauge_force (two-row loads)", tb, ta))
say("      " + ratio_line("the same with staple_recon = 0 in the improved sweep (18 reals per link)", tb18, ta))
say("      operation count per link: 73 products against 13 (5.6), 97 link loads against 19 (5.1)")
say("c.    " + ratio_line("lqcd_gauge_rectangle against lqcd_gauge_plaquette", tr, tp))
