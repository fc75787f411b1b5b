"""Every solver form on ill-conditioned systems against the oracle (tests/hard_systems.py: the systems, the accuracy contract and its derivation;
tests/golden/hard_systems.json: what the oracle's textbook solvers show on them; tests/test_cpu_hard_system_reference.py: the reference side).

The other solver tests run on hot links far from kappa_c, where a CG stops after ~76 iterations and the forms that replace the textbook recurrences --
the CG's residual ring, the merged BiCGStab update, the mixed-precision chains, the multi-shift solvers, the batched even-odd BiCGStab -- cannot show
their rounding.  Here the solution is 10^3 times the right-hand side and a solve runs 300 to 1800 iterations.  Every solve is held to

    t = |b - A x| (oracle)  <=  sqrt(rr_reported) + 8 max(C_ref, 0.25) u |A| |x|      and      rr_reported < eps = 1e-16

never to t^2 < eps, which a correct textbook CG misses on these rows.  CG forms take within 5 % of the oracle's iteration count; BiCGStab counts are
compared with nothing (erratic near kappa_c), the residual and the bit-equalities carry those cases.

Largest ratio (t - sqrt(rr_reported)) / (u |A| |x|) measured on the MI355X, per form (allowed: 8 max(C_ref, 0.25)); iterations; wall time of a solve:

    form                                                     row                    ratio   allowed   iterations (oracle)    solve
    CG cg_fused 0 / 1 / 2, cg_defer_x 0 / 4 / 8              wilson_cg_16           0.524   4.49      1073 (1073)            22 - 43 ms
    CG residual ring K = 2 / 4 / 8, tgauge 0 / 2             wilson_cg_16           0.559   4.49      1072 - 1073 (1073)     20 ms
    CG defaults (cg_small form), K = 8 under graph replay    wilson_cg_16           0.559   4.49      1073 (1073)            18 - 20 ms
    CG K = 8 from a Gaussian guess                           wilson_cg_16_x0        0.475   3.70      1073 (1073)            21 ms
    CG K = 8, x-share / sweep / centre hint on and off       wilson_cg_32           0.848   5.69      1793 (1792)            33 ms
    staggered CG, one launch and launch chain, stag_both     staggered_cg_16        0.029   2.00      624 (640)              5 - 10 ms
    staggered parity-block CG                                staggered_cg_16_even   0.017   2.00      623 (623)              17 ms
    shiftedcg, unshifted system                              wilson_multishift_16   0.496   3.84      1073 (1073)            25 ms
    shiftedcg / shiftedcg_mixed, shifted systems             wilson_multishift_16   < 0     2.00      (t < sqrt(eps) for every sigma: 9.3e-17 .. 9.9e-17 / <= 5.0e-17)
    shiftedcg_mixed, unshifted system                        wilson_multishift_16   < 0     3.84      2264 fp32, 8 corrections   51 ms
    mixed CG, mixed_pair32 0 / 1                             wilson_cg_16           0.003   4.49      1649 / 1664 fp32, 4 outer  33 - 39 ms
    even-odd BiCGStab bicg_fused 0 / 2 / 4 (guard 6, 0)      wilson_eo_D / Ddag     0.062   2.00      368 - 396 (411 / 406)  15 - 20 ms
    even-odd BiCGStab, fp32 chain, links16 x reliable        wilson_eo_D / Ddag     0.074   2.00      535 - 1200 fp32        20 - 51 ms
    batched even-odd BiCGStab, 4 unequal columns             wilson_eo_D gauss/pt   0.030   2.00      391, 316, 0, 138       29 ms

No form needs more than a ninth of its allowance; the forms that replace the textbook recurrences show the constant of the textbook CG (0.56).
The whole file takes 6 s on the device.

What the file found.  (i) bicg_mixed with fp32 links asked its first fp32 chain for 4.5e-6, below the floor rounding puts under an fp32 recurrence on
this system (about 5e-5): the chain wandered through all MaxCGstep iterations and left the fp64 chain that finishes the solve a budget of one --
NotConverged at residual 0.09.  The chain now stops when its residual sets no new low (mixed.hip inner_bicgstab_eo32); the cases below are the test.
(ii) The mixed-precision CG gives the action to first order in the residual only (test_action_through_the_mixed_precision_cg).
"""
import time

import numpy as np
import pytest

import hard_systems as hs
from f32_bound import no_handoff

pytestmark = pytest.mark.gpu

MAXIT = 6000
WILSON16, WILSON16_X0, WILSON32 = "wilson_cg_16", "wilson_cg_16_x0", "wilson_cg_32"


# ------------------------------------------------------------------ helpers
def wilson(lq, orc, name, tunables=(), method=None, maxit=MAXIT):
    """A fresh context with the row's links, operator and right-hand side; tunables: (key, value) pairs set before anything runs."""
    s = hs.system(name)
    lat = lq.Lattice(s["L"])
    for k, v in tunables:
        lat.set_param(k, v)
    U = lq.Gaugefields(lat).upload(hs.gauge(orc, s))
    p = {"Dirac_operator": "Wilson", "κ": s["kappa"], "boundarycondition": s["bc"], "eps_CG": s["eps"], "MaxCGstep": maxit}
    if method:
        p["method_CG"] = method
    D = lq.Dirac_operator(U, None, p)
    b = lq.Fermionfields(lat, lq.WILSON).upload(hs.rhs(orc, s))
    return s, lat, U, D, b


def staggered(lq, orc, name, tunables=()):
    s = hs.system(name)
    lat = lq.Lattice(s["L"])
    for k, v in tunables:
        lat.set_param(k, v)
    U = lq.Gaugefields(lat).upload(hs.gauge(orc, s))
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Staggered", "mass": s["mass"], "boundarycondition": s["bc"], "eps_CG": s["eps"], "MaxCGstep": MAXIT})
    b = lq.Fermionfields(lat, lq.STAGGERED).upload(hs.rhs(orc, s))
    return s, lat, U, D, b


def cg(lq, orc, s, D, b, x0h=None):
    """(x, iterations, reported rr) of solve_DinvX_ on D^+D; prints the wall time of the solve."""
    x = b.similar()
    if x0h is not None:
        x.upload(x0h)
    else:
        lq.clear_fermion_(x)
    t0 = time.perf_counter()
    it, rr = lq.solve_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
    print("%s: %d iterations in %.3f s" % (s["name"], it, time.perf_counter() - t0))
    return x.download(), it, rr


def hold(orc, s, xh, rr, label, sigma=0.0, shift=None, dagger=None, b=None):
    """The accuracy contract for one downloaded solution; b: a right-hand side other than the row's (a column held to the row's C_ref)."""
    t2 = hs.true_rr(orc, s, xh, sigma, dagger, b)
    ok, c = hs.meets(s, t2, rr, float(np.linalg.norm(xh)), sigma, shift, label=label)
    assert ok, (s["name"], label, "ratio", c, "true rr", t2, "reported", rr)
    return c


def count_in_band(s, it, label=""):
    ref = hs.fixture()[s["name"]]["iterations"]
    print("%s %s iterations %d, oracle %d (%+.2f %%)" % (s["name"], label, it, ref, 100.0 * (it - ref) / ref))
    assert abs(it - ref) <= 0.05 * ref, (s["name"], label, it, ref)


# ------------------------------------------------------------------ 1. the CG forms, 16.8.8.4, kappa 0.1285
# (id, tunables, cg_rring_active)
CG_FORMS = [
    ("reference", (("cg_fused", 0),), 0),
    ("norm_fused", (("cg_fused", 1),), 0),
    ("fused", (("cg_fused", 2), ("cg_defer_x", 0)), 0),
    ("defer_x4", (("cg_fused", 2), ("cg_defer_x", 4)), 0),
    ("defer_x8", (("cg_fused", 2), ("cg_defer_x", 8)), 0),
    ("rring2", (("cg_fused", 3), ("cg_rring", 2)), 2),
    ("rring4", (("cg_fused", 3), ("cg_rring", 4)), 4),
    ("rring8", (("cg_fused", 3), ("cg_rring", 8)), 8),
]


@pytest.mark.parametrize("tg", [0, 2])
@pytest.mark.parametrize("form", CG_FORMS, ids=[f[0] for f in CG_FORMS])
def test_cg_forms(lq, orc, form, tg):
    name, tun, K = form
    s, lat, U, D, b = wilson(lq, orc, WILSON16, (("cg_persist", 0), ("cg_small", 0), ("cg_tgauge", tg)) + tun)
    xh, it, rr = cg(lq, orc, s, D, b)
    assert lat.get_param("cg_rring_active") == K and lat.get_param("tgauge_active") == (1 if tg else 0)
    hold(orc, s, xh, rr, "cg %s tgauge %d" % (name, tg))
    count_in_band(s, it, name)
    assert np.array_equal(b.download(), hs.rhs(orc, s))


def test_cg_defaults_untouched(lq, orc):
    s, lat, U, D, b = wilson(lq, orc, WILSON16)
    xh, it, rr = cg(lq, orc, s, D, b)
    print("defaults: cg_fused %d cg_small %d cg_rring_active %d tgauge_active %d" % tuple(lat.get_param(k) for k in ("cg_fused", "cg_small", "cg_rring_active", "tgauge_active")))
    hold(orc, s, xh, rr, "cg defaults")
    count_in_band(s, it, "defaults")


def test_cg_ring_graph_replay(lq, orc):
    s, lat, U, D, b = wilson(lq, orc, WILSON16, (("cg_persist", 0), ("cg_small", 0), ("cg_tgauge", 2), ("cg_fused", 3), ("cg_rring", 8)))
    out = []
    for graph in (0, 1):
        lat.set_param("graph", graph)
        out.append(cg(lq, orc, s, D, b))
        assert lat.get_param("cg_rring_active") == 8 and lat.get_param("tgauge_active") == 1
    lat.set_param("graph", 0)
    hold(orc, s, out[1][0], out[1][2], "cg rring8 graph")
    count_in_band(s, out[1][1], "rring8 graph")
    assert out[0][1] == out[1][1] and np.array_equal(out[0][0], out[1][0])      # a replayed burst is the same launches


def test_cg_non_zero_start(lq, orc):
    s, lat, U, D, b = wilson(lq, orc, WILSON16_X0, (("cg_persist", 0), ("cg_small", 0), ("cg_tgauge", 2), ("cg_fused", 3), ("cg_rring", 8)))
    xh, it, rr = cg(lq, orc, s, D, b, hs.guess(orc, s))
    assert lat.get_param("cg_rring_active") == 8
    hold(orc, s, xh, rr, "cg rring8 x0")
    count_in_band(s, it, "rring8 x0")


def test_an_exhausted_hard_solve_raises_and_equals_the_fixed_window(lq, orc):
    s, lat, U, D, b = wilson(lq, orc, WILSON16, (("cg_persist", 0), ("cg_small", 0), ("cg_tgauge", 2), ("cg_fused", 3), ("cg_rring", 8)), maxit=500)
    x = b.similar()
    lq.clear_fermion_(x)
    with pytest.raises(lq.NotConverged):
        lq.solve_DinvX_(x, lq.DdagD_operator(D), b)
    assert lat.get_param("cg_rring_active") == 8
    w = b.similar()
    lq.clear_fermion_(w)
    lq.lib.check(lq.lib.lib().lqcd_solve_cg_DdagD_fixed(D._h, w._h, b._h, 500))
    xh = x.download()
    assert np.isfinite(xh).all() and np.array_equal(xh, w.download())


# ------------------------------------------------------------------ 2. x-share, reversed sweep, streaming hint: 32.4.8.4, ~1800 iterations, bit for bit
@pytest.mark.parametrize("key,active", [("dslash_xshare", "xshare_active"), ("cg_sweep_alt", "cg_sweep_alt_active"), ("nt_centre", None)])
def test_switches_that_promise_the_same_bits(lq, orc, key, active):
    s, lat, U, D, b = wilson(lq, orc, WILSON32, (("cg_persist", 0), ("cg_small", 0), ("cg_tgauge", 2), ("cg_fused", 3), ("cg_rring", 8)))
    out = []
    for v in (0, 1):
        lat.set_param(key, v)
        out.append(cg(lq, orc, s, D, b))
        assert lat.get_param("cg_rring_active") == 8 and lat.get_param("tgauge_active") == 1
        if active:
            assert lat.get_param(active) == v, (key, v)
        if key != "dslash_xshare":
            assert lat.get_param("xshare_active") == 1      # XH = 16: the default takes the x-share
        hold(orc, s, out[-1][0], out[-1][2], "cg rring8 %s %d" % (key, v))
        count_in_band(s, out[-1][1], "%s %d" % (key, v))
    assert out[0][1] == out[1][1], (key, out[0][1], out[1][1])
    assert np.array_equal(out[0][0], out[1][0]), key


# ------------------------------------------------------------------ 3. staggered, m = 0.005
@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("both", [0, 1])
def test_staggered_cg(lq, orc, both, persist):
    """Default form; cg_persist = 1 (default) is the one-launch solve on this lattice (64 workgroups), which switches itself off if it gives up."""
    s, lat, U, D, b = staggered(lq, orc, "staggered_cg_16", (("stag_both", both), ("cg_persist", persist)))
    xh, it, rr = cg(lq, orc, s, D, b)
    assert lat.get_param("cg_persist") == persist and lat.get_param("stag_both") == both
    hold(orc, s, xh, rr, "staggered cg stag_both %d cg_persist %d" % (both, persist))
    count_in_band(s, it, "stag_both %d cg_persist %d" % (both, persist))


def test_staggered_parity_block_solve(lq, orc):
    s, lat, U, D, b = staggered(lq, orc, "staggered_cg_16_even")
    even = hs.even_mask(s["L"])
    marker = np.array(orc.gaussian_spinor(hs.shape(orc, s), 943))
    marker[even, :] = 0.0                                       # zero guess on the solved parity, a marker on the other
    x = lq.Fermionfields(lat, lq.STAGGERED).upload(marker)
    t0 = time.perf_counter()
    it, rr = lq.solve_parity_DinvX_(x, lq.DdagD_operator(D), b, 0, return_info=True)
    print("%s: %d iterations in %.3f s" % (s["name"], it, time.perf_counter() - t0))
    got = x.download()
    assert np.array_equal(got[~even, :], marker[~even, :])      # the other half is left alone
    got[~even, :] = 0.0
    hold(orc, s, got, rr, "staggered parity block")
    count_in_band(s, it, "parity block")


# ------------------------------------------------------------------ 4. multi-shift
@pytest.mark.parametrize("mixed", [0, 1], ids=["shiftedcg", "shiftedcg_mixed"])
def test_multishift(lq, orc, mixed):
    s, lat, U, D, b = wilson(lq, orc, "wilson_multishift_16")
    A = lq.DdagD_operator(D)
    xs = [b.similar() for _ in s["sigmas"]]
    x = b.similar()
    t0 = time.perf_counter()
    if mixed:
        it, outer, rr = lq.shiftedcg_mixed(xs, list(s["sigmas"]), x, A, b, return_info=True)
        print("shiftedcg_mixed: %d fp32 iterations, %d correction solves, largest true rr %.4e, %.3f s" % (it, outer, rr, time.perf_counter() - t0))
        no_handoff(lat, "shiftedcg_mixed")      # ill-conditioned, eps = 1e-16: more correction solves, none of them handed to the fp64 solver
    else:
        it, rr = lq.shiftedcg(xs, list(s["sigmas"]), x, A, b, return_info=True)
        print("shiftedcg: %d iterations in %.3f s" % (it, time.perf_counter() - t0))
        count_in_band(s, it, "shiftedcg")
    form = "shiftedcg_mixed" if mixed else "shiftedcg"
    hold(orc, s, x.download(), rr, form + " sigma 0")
    for j, sigma in enumerate(s["sigmas"]):
        hold(orc, s, xs[j].download(), rr, form + " sigma %g" % sigma, sigma=sigma, shift=j)


# ------------------------------------------------------------------ 5. mixed-precision CG
@pytest.mark.parametrize("pair32", [0, 1])
def test_mixed_cg(lq, orc, pair32):
    """The header of lqcd_solve_mixed_cg_DdagD promises the true fp64 residual below eps: held to the allowance of the fp64 forms."""
    s, lat, U, D, b = wilson(lq, orc, WILSON16, (("mixed_pair32", pair32),))
    x = b.similar()
    lq.clear_fermion_(x)
    t0 = time.perf_counter()
    it, outer, rr = lq.solve_mixed_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
    print("mixed cg pair32 %d: %d inner iterations, %d outer corrections, reported true rr %.4e, %.3f s" % (pair32, it, outer, rr, time.perf_counter() - t0))
    assert lat.get_param("pair32_active") == pair32
    no_handoff(lat, "mixed cg pair32 %d" % pair32)
    hold(orc, s, x.download(), rr, "mixed cg pair32 %d" % pair32)


# ------------------------------------------------------------------ 6. even-odd BiCGStab, kappa 0.128
# (id, tunables, bicg_xrp_active)
BICG_FORMS = [
    ("generic", (("bicg_fused", 0),), 0),
    ("fused2", (("bicg_fused", 2),), 0),
    ("merged_guard6", (("bicg_fused", 4), ("bicg_rec_guard", 6)), 2),
    ("merged_guard0", (("bicg_fused", 4), ("bicg_rec_guard", 0)), 2),
]


def eo_solve(lq, s, D, b):
    Dd = D.adjoint() if s["dagger"] else D
    Dd.method_CG = "bicgstab_evenodd"
    x = b.similar()
    lq.clear_fermion_(x)
    t0 = time.perf_counter()
    it, rr = lq.solve_DinvX_(x, Dd, b, return_info=True)
    print("%s: %d iterations in %.3f s" % (s["name"], it, time.perf_counter() - t0))
    assert 0 < it < MAXIT
    return x.download(), it, rr


@pytest.mark.parametrize("row", ["wilson_eo_D_gauss", "wilson_eo_Ddag_gauss"])
@pytest.mark.parametrize("form", BICG_FORMS, ids=[f[0] for f in BICG_FORMS])
def test_evenodd_bicgstab_forms(lq, orc, form, row):
    name, tun, xrp = form
    s, lat, U, D, b = wilson(lq, orc, row, tun, method="bicgstab_evenodd")
    xh, it, rr = eo_solve(lq, s, D, b)
    assert lat.get_param("bicg_xrp_active") == xrp
    hold(orc, s, xh, rr, "bicgstab_eo %s" % name, dagger=s["dagger"])      # the residual of the FULL system b - D x


@pytest.mark.parametrize("row", ["wilson_eo_D_gauss", "wilson_eo_Ddag_gauss"])
@pytest.mark.parametrize("links16,reliable", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_evenodd_bicgstab_mixed_chain(lq, orc, links16, reliable, row):
    s, lat, U, D, b = wilson(lq, orc, row, (("bicg_mixed", 1), ("mixed_links16", links16), ("bicg_reliable", reliable)), method="bicgstab_evenodd")
    xh, it, rr = eo_solve(lq, s, D, b)
    assert lat.get_param("pair32_active") == 1
    no_handoff(lat, "bicgstab_eo mixed links16 %d reliable %d" % (links16, reliable))
    hold(orc, s, xh, rr, "bicgstab_eo mixed links16 %d reliable %d" % (links16, reliable), dagger=s["dagger"])


# ------------------------------------------------------------------ 7. the batched even-odd BiCGStab with unequal columns
def test_batched_bicgstab_with_unequal_columns(lq, orc):
    """Gaussian, point source, zero, and the Gaussian scaled by 1e-6 -- which meets the absolute eps 250 iterations before the first and sits frozen the
    longest.  A frozen column must not move: every column of the four-column call is the bits of the same column solved alone by the batched solver.
    Against the single-column bicgstab_evenodd with bicg_fused = 2 the batched solver is the same recurrences with the same partial sums except for the
    two inner products against r0, whose partials it sums in another order (include/lqcd_hip.h promises agreement to solver accuracy, not bits): the
    point source, where r0 has a single entry and those two sums have one term, is the same bits over its 316 iterations, and so is the zero column; the
    Gaussian columns take another rounding path through a system this ill-conditioned (measured: 391 against 396 iterations, largest entry of the
    difference 1.1e-9 of the largest entry of x; the scaled column 138 against 138 and 8.3e-6 -- its eps is a relative 1e-9) and are held by the
    accuracy contract alone."""
    sg, sp = hs.system("wilson_eo_D_gauss"), hs.system("wilson_eo_D_point")
    s, lat, U, D, b = wilson(lq, orc, "wilson_eo_D_gauss", method="bicgstab_evenodd")
    g, pt = hs.rhs(orc, sg), hs.rhs(orc, sp)
    cols = [np.array(g), np.array(pt), np.zeros_like(g), 1e-6 * g]
    rows = [sg, sp, sg, sg]
    bs = [lq.Fermionfields(lat, lq.WILSON).upload(c) for c in cols]
    xs = [c.similar() for c in bs]
    for x in xs:
        lq.clear_fermion_(x)
    t0 = time.perf_counter()
    its, rrs = lq.solve_DinvX_multi_(xs, D, bs, return_info=True)
    print("batched: iterations", its, "reported rr", rrs, "%.3f s" % (time.perf_counter() - t0))
    assert lat.get_param("mrhs_active") == 4
    sol = [x.download() for x in xs]
    assert its[2] == 0 and rrs[2] == 0.0 and not sol[2].any()                  # the zero column stays exactly zero
    assert its[3] < its[0] - 100 and all(0 < its[j] < MAXIT for j in (0, 1, 3))
    for j in (0, 1, 3):
        hold(orc, rows[j], sol[j], rrs[j], "batched column %d" % j, dagger=False, b=cols[j])
    for c, bj in zip(cols, bs):
        assert np.array_equal(bj.download(), c)
    lat.set_param("bicg_fused", 2)
    for j in range(4):
        alone = bs[j].similar()
        lq.clear_fermion_(alone)
        it1, rr1 = lq.solve_DinvX_multi_([alone], D, [bs[j]], return_info=True)
        assert lat.get_param("mrhs_active") == 1
        assert it1[0] == its[j] and rr1[0] == rrs[j] and np.array_equal(alone.download(), sol[j]), (j, it1, its[j])
        single = bs[j].similar()
        lq.clear_fermion_(single)
        its1, rrs1 = lq.solve_DinvX_(single, D, bs[j], return_info=True)
        sh = single.download()
        same = bool(np.array_equal(sh, sol[j]))
        err = float(np.abs(sh - sol[j]).max() / max(np.abs(sh).max(), 1e-300))
        print("  column %d against the single-column solve (bicg_fused 2): iterations %d / %d, same bits %s, rel max diff %.3e" % (j, its[j], its1, same, err))
        assert lat.get_param("bicg_xrp_active") == 0
        if j in (1, 2):
            assert same and its1 == its[j], (j, its1, its[j], err)


# ------------------------------------------------------------------ 8. action and force through a hard solve
# the oracle at eps = 1e-16 against the oracle at eps = 1e-20 (8 threads): |dS| / S = 8.49e-15, max |dG| / max |G| = 7.60e-12; the library gets 4 x that
ACTION_BOUND, FORCE_BOUND = 4 * 8.4892e-15, 4 * 7.6012e-12
_action_ref = {}


def action_reference(orc, s):
    if not _action_ref:
        before = orc.lib().orc_get_threads()
        orc.set_threads(hs.THREADS)
        try:
            S, X, Y, it, st = orc.fermi_action(orc.WILSON, hs.gauge(orc, s), hs.rhs(orc, s), s["L"], s["kappa"], 1.0, s["bc"], eps=1e-20, maxiter=MAXIT)
            assert st == 0
            _action_ref["S"], _action_ref["G"] = S, orc.fermion_force(orc.WILSON, hs.gauge(orc, s), X, Y, s["L"], s["kappa"], 1.0, s["bc"])
        finally:
            orc.set_threads(before)
    return _action_ref["S"], _action_ref["G"]


def action_and_force(lq, orc, mixed, eo):
    s, lat, U, D, b = wilson(lq, orc, WILSON16, (("mixed_action_solver", mixed), ("action_eo_solver", eo)))
    Sref, Gref = action_reference(orc, s)
    fa = lq.FermiAction(D, {"Nf": 2})
    t0 = time.perf_counter()
    S, it = lq.evaluate_FermiAction(fa, U, b, return_info=True)
    G = lq.Gaugefields(lat)
    lq.calc_UdSfdU_(G, fa, U, b)
    dt = time.perf_counter() - t0
    Xh, Yh, Gh = fa._temporary_fermionfields[0].download(), fa._temporary_fermionfields[1].download(), G.download()
    dS = abs(S - Sref) / abs(Sref)
    dG = float(np.abs(Gh - Gref).max() / np.abs(Gref).max())
    print("action mixed_action_solver %d action_eo_solver %d: %d iterations, S %.15e (oracle %.15e) rel diff %.3e (bound %.3e); force rel max diff %.3e (bound %.3e); %.3f s"
          % (mixed, eo, it, S, Sref, dS, ACTION_BOUND, dG, FORCE_BOUND, dt))
    assert lat.get_param("mixed_action_solver") == mixed and lat.get_param("action_eo_solver") == eo
    assert lat.get_param("pair32_active") == mixed              # a fresh context: an fp32 operator was set up if and only if a mixed solver ran
    if mixed and not eo:
        no_handoff(lat, "action through the mixed CG")      # (the solve of the force evaluation, the last one)
    elif mixed:
        # by design: at this kappa the fp32 chain of the first even-odd solve stalls, bicgstab_eo_wilson_mixed hands the Schur system to the fp64 chain -- once per
        # solve -- which stalls as well; the second even-odd solve is then not tried and the fp64 CG on the normal equations (no mixed solver) finishes
        print("action eo mixed: mixed_handoffs %d mixed_fp64_iters %d" % (lat.get_param("mixed_handoffs"), lat.get_param("mixed_fp64_iters")))
        assert lat.get_param("mixed_handoffs") == 1 and lat.get_param("mixed_fp64_iters") > 0
    fa.close()
    return s, it, S, Sref, dS, dG, Xh, Yh, Gh


@pytest.mark.parametrize("mixed,eo", [(0, 1), (1, 1), (0, 0)])
def test_action_and_force_through_a_hard_solve(lq, orc, mixed, eo):
    """evaluate_FermiAction and calc_UdSfdU_ (Wilson, Nf = 2, kappa 0.1285, eps 1e-16) against orc.fermi_action / orc.fermion_force at eps 1e-20.
    No bound follows from first principles; measured: the oracle at eps 1e-16 differs from the oracle at eps 1e-20 by 8.49e-15 in S (relative) and by
    7.60e-12 in the force (largest entry, relative to the largest entry).  The library is given 4 x that: 3.40e-14 and 3.04e-11 (measured on the
    device: 2.95e-15 and 8.10e-12).
    action_eo_solver = 1 (default) asks for two even-odd BiCGStab solves; at this kappa they stall (fp64 and, with mixed_action_solver = 1, the fp32
    chain alike) and the CG on the normal equations finishes: the iteration count returned is then the CG's.  action_eo_solver = 0 is the CG directly."""
    s, it, S, Sref, dS, dG, Xh, Yh, Gh = action_and_force(lq, orc, mixed, eo)
    if not eo:
        count_in_band(s, it, "action CG")
    assert dS <= ACTION_BOUND and dG <= FORCE_BOUND, (dS, dG)


def test_action_through_the_mixed_precision_cg(lq, orc):
    """mixed_action_solver = 1 with action_eo_solver = 0: the solve is the mixed-precision CG, so that this solver of the action is reached whatever the
    even-odd route does.  Its X meets the accuracy contract, but a defect correction's residual is not orthogonal to the solution the way a single CG's
    is: S = eta^+ X is then accurate to FIRST order in the residual, |S - S_exact| = |X_exact^+ r| <= |X| t, where the CG from zero is accurate to
    second order.  Measured: |dS| / S = 4.96e-11 (CG: 2.95e-15; the first-order bound |X| t / S is 7.3e-10), force 1.49e-10 of the largest entry
    (CG: 8.10e-12) -- outside 4 x the oracle's own difference, inside what a true residual below eps promises.  Held to the first-order bound; the
    force sweep is held on the solver's own X and Y at the 1e-12 of the force tests (bilinear in fields of norm 1e6)."""
    s, it, S, Sref, dS, dG, Xh, Yh, Gh = action_and_force(lq, orc, 1, 0)
    t2, xnorm = hs.true_rr(orc, s, Xh), float(np.linalg.norm(Xh))
    print("mixed cg action: true rr %.4e |X| %.4e" % (t2, xnorm))
    assert np.sqrt(t2) <= np.sqrt(s["eps"]) + hs.allowance(s, xnorm), t2      # (the action reports no residual: eps stands for it)
    first_order = xnorm * np.sqrt(t2) / abs(Sref)
    print("mixed cg action: |X| t / S = %.3e, measured %.3e" % (first_order, dS))
    assert dS <= first_order + ACTION_BOUND, (dS, first_order)
    Go = orc.fermion_force(orc.WILSON, hs.gauge(orc, s), Xh, Yh, s["L"], s["kappa"], 1.0, s["bc"])
    assert float(np.abs(Gh - Go).max() / np.abs(Go).max()) <= 1e-12
    # Y = D X at the 1e-13 of the operator tests, on the scale of what D is applied to (X is almost a null vector: |Y| is 1e-4 |X|)
    assert float(np.abs(Yh - hs.apply_A(orc, s, Xh, dagger=False)).max()) <= 1e-13 * hs.norm_A(s, dagger=False) * float(np.abs(Xh).max())
