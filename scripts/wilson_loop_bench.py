"""R x T Wilson loops at 32^3x64 (hot start, thermalised by three flow steps): wall time of the 4 x 4 table (the reference's default Rmax = Tmax = 4)
and of the 16 x 32 table (lqcd_gauge_wilson_loops), with lqcd_gauge_plaquette timed in the same run as the yardstick.  The bytes the kernels request are
counted from the shapes: per R the extend sweep reads the three space-like links (and, for R > 1, the three lines) and writes the three lines; the walk
reads per (site, mu) the line once and per T two time-like links and one line (3 x 144 B).  Compulsory per R: the time-like links once plus the three
line fields once = 576 B/site.  Wall times per call here; the kernel times come from running it under rocprofv3 --kernel-trace --stats.
usage: wilson_loop_bench.py [reps]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import latticeqcd_jl_amd as lq  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
L = (32, 32, 32, 64)
PEAK = 8.0e12       # HBM bytes/s of the MI355X (data sheet)
U = lq.Initialize_Gaugefields(3, 0, *L, condition="hot", randomseed=111)
lat = U.lattice
lq.flow_(U, lq.Gradientflow(U, Nflow=3, eps=0.01))


def timed(fn, n):
    fn()
    lat.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    lat.sync()
    return 1e3 * (time.perf_counter() - t0) / n


def requested_bytes_per_site(Rmax, Tmax):
    extend = 864 + (Rmax - 1) * 1296              # R = 1: 3 links in, 3 lines out; R > 1: 3 lines + 3 links in, 3 lines out
    walk = Rmax * 3 * 144 * (1 + 3 * Tmax)
    return extend, walk


V = L[0] * L[1] * L[2] * L[3]
print(f"lattice {L}  reps {reps}")
plaq = timed(lambda: lq.calculate_Plaquette(U), reps)
print(f"plaquette (lqcd_gauge_plaquette), the yardstick    {plaq:9.3f} ms wall   ({V * 576 / 1e9:.3f} GB compulsory: the links once)")
for Rmax, Tmax in ((4, 4), (16, 32)):
    ms = timed(lambda: lq.wilson_loops(U, Rmax, Tmax), reps if Rmax == 4 else max(1, reps // 3))
    ext, walk = requested_bytes_per_site(Rmax, Tmax)
    req, comp = V * (ext + walk), V * 576 * Rmax
    print(f"{Rmax:2d} x {Tmax:2d} table (lqcd_gauge_wilson_loops)            {ms:9.3f} ms wall   {ms / Rmax:8.3f} ms per R   {1e3 * ms / (Rmax * Tmax):8.1f} us per (R, T)"
          f"   = {ms / plaq:.1f} plaquette calls")
    print(f"    requested {req / 1e9:9.3f} GB (extend {V * ext / 1e9:.3f} + walk {V * walk / 1e9:.3f}; {(ext + walk) / (Rmax * Tmax):.0f} B/site per (R, T))"
          f" -> {req / (1e-3 * ms) / 1e12:.3f} TB/s = {req / (1e-3 * ms) / PEAK:.3f} of 8 TB/s")
    print(f"    compulsory {comp / 1e9:8.3f} GB (576 B/site per R) -> {comp / (1e-3 * ms) / 1e12:.3f} TB/s = {comp / (1e-3 * ms) / PEAK:.3f} of 8 TB/s")
tab = lq.wilson_loops(U, 4, 4)
print("W(R, T), R, T = 1..4:")
for row in tab:
    print("   ", " ".join(f"{v: .10e}" for v in row))
print("Creutz ratios:", " ".join(f"{v:.6f}" for v in lq.creutz_ratios(tab).ravel()))
