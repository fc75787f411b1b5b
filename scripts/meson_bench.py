"""Meson correlators at 32^3x64, kappa = 0.12 (hot start, smoothed by three flow steps): wall times of
  - lqcd_meson_contract of 12 resident point-source columns,
  - twelve lqcd_norm2 calls on the same columns -- the yardstick: the same 4.83 GB read once with trivial arithmetic,
  - lqcd_meson_correlators as a whole (12 solves + 3 contractions),
  - the 12 lqcd_solve_bicgstab_eo calls alone,
  - the host route of tests/test_gpu_quenched_literature.py: 12 downloads + the numpy sum of |S|^2,
and the fraction of 8 TB/s the contraction reaches on its 2304 compulsory bytes per site (12 columns x 192 B).  Kernel times come from running it under
rocprofv3 --kernel-trace --stats.
usage: meson_bench.py [reps]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import latticeqcd_jl_amd as lq  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
L = (32, 32, 32, 64)
KAPPA = 0.12
PEAK = 8.0e12       # HBM bytes/s of the MI355X (data sheet)
U = lq.Initialize_Gaugefields(3, 0, *L, condition="hot", randomseed=111)
lat = U.lattice
lq.flow_(U, lq.Gradientflow(U, Nflow=3, eps=0.01))
D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "r": 1.0, "eps_CG": 1e-19, "MaxCGstep": 3000, "method_CG": "bicgstab_evenodd"})
b = lq.Fermionfields(lat, lq.WILSON)
cols = [lq.Fermionfields(lat, lq.WILSON) for _ in range(12)]
src = (0, 0, 0, 0)


def solves():
    its = []
    for ic in range(3):
        for isp in range(4):
            lq.setindex_global_(b, ic, *src, isp)
            lq.clear_fermion_(cols[4 * ic + isp])
            its.append(lq.solve_DinvX_(cols[4 * ic + isp], D, b, return_info=True)[0])
    return its


def norms():
    n2 = C.c_double(0)
    for c in cols:
        lq.check(lq.lib.lib().lqcd_norm2(c._h, C.byref(n2)))


def host_route():
    Cpi = np.zeros(L[3])
    buf = np.zeros(lat.fermion_shape(lq.WILSON), dtype=np.complex128)
    for c in cols:
        c.download(into=buf)
        Cpi += (buf.real ** 2 + buf.imag ** 2).sum(axis=(0, 2, 3, 4, 5))
    return Cpi


def timed(fn, n):
    fn()
    lat.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    lat.sync()
    return 1e3 * (time.perf_counter() - t0) / n


V = L[0] * L[1] * L[2] * L[3]
gb = V * 2304 / 1e9
print(f"lattice {L}  kappa {KAPPA}  reps {reps}  plaquette {lq.calculate_Plaquette(U):.6f}")
its = solves()
print("iterations of the 12 solves:", its)
t_solve = timed(solves, reps)
nfast = 30 * reps       # the sub-millisecond calls are timed over windows of a few tenths of a second, three rounds each in alternation; the medians are reported
rounds = [(timed(lambda: lq.meson_contract(cols), nfast), timed(norms, nfast), timed(lambda: [lq.norm2_timeslices(c) for c in cols], nfast)) for _ in range(3)]
for k, r in enumerate(rounds):
    print(f"round {k}: meson_contract {r[0]:.4f} ms   twelve lqcd_norm2 {r[1]:.4f} ms   twelve norm2_timeslices {r[2]:.4f} ms")
t_contract, t_norm, t_slices = (float(np.median([r[j] for r in rounds])) for j in range(3))
t_all = timed(lambda: lq.meson_correlators(D, src), reps)
t0 = time.perf_counter()
Cpi_host = host_route()
t_host = 1e3 * (time.perf_counter() - t0)
tab = lq.meson_contract(cols)
print(f"meson_contract, 12 resident columns                {t_contract:10.3f} ms wall   {gb:.3f} GB compulsory -> {gb / t_contract:.3f} TB/s = {gb * 1e9 / (1e-3 * t_contract) / PEAK:.3f} of 8 TB/s")
print(f"twelve lqcd_norm2 calls, the yardstick             {t_norm:10.3f} ms wall   {gb:.3f} GB -> {gb / t_norm:.3f} TB/s;  contract / yardstick = {t_contract / t_norm:.2f} (target <= 3)")
print(f"twelve lqcd_spinor_norm2_timeslices calls          {t_slices:10.3f} ms wall")
print(f"meson_correlators as a whole                       {t_all:10.3f} ms wall")
print(f"the 12 lqcd_solve_bicgstab_eo calls alone          {t_solve:10.3f} ms wall   ({t_all - t_solve:.3f} ms on top of them in the measurement)")
print(f"host route: 12 downloads + numpy sum |S|^2         {t_host:10.3f} ms wall   = {t_host / t_contract:.0f} contractions")
print("max |C_15 (device) / C_pi (host) - 1| =", float(np.abs(tab[15] / Cpi_host - 1.0).max()))
full = lq.meson_correlators(D, src)
print("max |meson_correlators - meson_contract| / C_15 =", float((np.abs(full - tab) / tab[15]).max()))
for n in (0, 1, 8, 15):
    print(f"C_{n:<2d} ({lq.MESON_CHANNELS[n]:>8s}) t = 0..7:", " ".join(f"{v: .6e}" for v in tab[n, :8]))
