"""The temporal-gauge Wilson CG on 8 reals per link (tunable cg_tgauge_recon = 8; fields.hip tgauge8_encode / tgauge8_gate, lqcd_internal.h link8_decode, stencil.hip
wilson_dirsplit_s_tg8, cg.hip cg_tgauge8_links).  16.8.8.4 (the smallest lattice that runs ring + temporal gauge; one seam in four slices) and 16.16.16.8, hot-start links,
boundary conditions (1,1,1,-1) and (1,1,1,1); cg_tgauge = 2, cg_rring_mult, cg_store_keep_mb and cg_tgauge_recon are all set explicitly (below 1025 stencil workgroups none of
them is on by default).

The 8-real solve is another operator than the 12-real one: its links are decode(encode(U')), within the gate (1e-14) of U'.  What that does to a CG window is taken from the
oracle, not from the code under test: the oracle's fixed-length CG on the rotated links and on tests/link8_numpy.py's decode(encode(.)) of them, same lattice, window and right-hand
side; the device's 8-real window may differ from its 12-real one by 10 x that (the margin covers the device's other summation order and encoder rounding).  Window: 3 d + 5
iterations, d the depth of the residual ring.

Measured on the MI355X (relative max-norm difference of x after the window, d = 8, 29 iterations; the gate is lqcd_gauge_tgauge8_deviation):
  lattice      bc            oracle 12 vs 8    device 12 vs 8    device gate
  16.8.8.4     (1,1,1,-1)    7.12e-16          8.81e-16          3.05e-15
  16.8.8.4     (1,1,1,1)     7.01e-16          7.62e-16          3.05e-15
  16.16.16.8   (1,1,1,-1)    7.67e-16          9.15e-16          2.19e-15
  16.16.16.8   (1,1,1,1)     7.57e-16          9.79e-16          2.19e-15
The 8-real solve to eps 1e-16 stops on the oracle's iteration (67, 67, 70, 70) with x within 1.1e-15 .. 1.8e-15 of the oracle's.  32.8.8.4 is added for the switch test
alone: the x-share and the y-share need XH = 16, on the two 16-wide lattices their keys change no launch.
"""
import numpy as np
import pytest

import link8_numpy as l8
from test_tgauge_oracle import gmul, rotate, sw

pytestmark = pytest.mark.gpu

KAPPA = 0.141139
SMALL = (16, 8, 8, 4)
MID = (16, 16, 16, 8)
WIDE = (32, 8, 8, 4)      # XH = 16: the lattice width at which the x-share and the y-share exist (the switch test only)
ANTI, PERIODIC = (1, 1, 1, -1), (1, 1, 1, 1)
MULT = 1              # cg_rring_mult: ring depth d = cg_rring x MULT
KEEP_MB = 1           # cg_store_keep_mb: on, a few slabs of these lattices
_cache = {}


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def make(lq, L, bc, Uh, bh, recon=8, eps=1e-16):
    lat = lq.Lattice(L)
    for k, v in (("cg_persist", 0), ("cg_small", 0), ("cg_tgauge", 2), ("cg_rring_mult", MULT), ("cg_store_keep_mb", KEEP_MB), ("cg_tgauge_recon", recon)):
        lat.set_param(k, v)
    U = lq.Gaugefields(lat).upload(Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": bc, "eps_CG": eps, "MaxCGstep": 3000})
    b = lq.Fermionfields(lat, lq.WILSON).upload(bh)
    return lat, U, D, b


def window(lq, lat, D, b, n):
    """x after n CG iterations from zero (n = None: the solve to eps); returns (x, iterations, tgauge_recon_active)"""
    x = b.similar()
    it = n
    if n is None:
        it, rr = lq.solve_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
    else:
        lq.lib.check(lq.lib.lib().lqcd_solve_cg_DdagD_fixed(D._h, x._h, b._h, int(n)))
    assert lat.get_param("tgauge_active") == 1
    return x.download(), it, lat.get_param("tgauge_recon_active")


def problem(orc, L, seed=811):
    """links, right-hand side: computed once per lattice, never written"""
    if ("p", L) not in _cache:
        _cache[("p", L)] = (orc.hot_gauge(L, seed), orc.gaussian_spinor(orc.wilson_shape(L), seed + 1))
    return _cache[("p", L)]


def oracle_pair(orc, L, bc, n):
    """relative max-norm difference of the oracle's n-iteration CG on the rotated links and on decode(encode(.)) of them"""
    key = ("o", L, bc, n)
    if key not in _cache:
        Uh, bh = problem(orc, L)
        G, Ug, gate, unit = rotate(Uh)
        assert gate <= 1e-14 and unit <= 1e-14
        U8 = np.ascontiguousarray(sw(l8.decode(l8.encode(sw(Ug)))))
        assert abs(U8 - Ug).max() <= 1e-14
        gb = gmul(G, bh)
        x12 = orc.cg_DdagD_fixed(orc.WILSON, Ug, gb, L, KAPPA, 1.0, bc, niter=n)
        x8 = orc.cg_DdagD_fixed(orc.WILSON, U8, gb, L, KAPPA, 1.0, bc, niter=n)
        _cache[key] = relmax(x8, x12)
    return _cache[key]


@pytest.mark.parametrize("bc", [ANTI, PERIODIC])
@pytest.mark.parametrize("L", [SMALL, MID])
def test_window_against_12_reals_within_the_oracle_bound_and_the_solve_against_the_oracle(lq, orc, L, bc):
    Uh, bh = problem(orc, L)
    lat, U, D, b = make(lq, L, bc, Uh, bh, recon=8)
    dev = lq.tgauge8_deviation(U)
    _, _, act = window(lq, lat, D, b, 1)
    d = lat.get_param("cg_rring_depth_active")
    assert act == 8 and d == lat.get_param("cg_rring") * MULT and d >= 2
    assert dev <= 1e-14, dev
    n = 3 * d + 5
    x8, _, act8 = window(lq, lat, D, b, n)
    s8, it8, _ = window(lq, lat, D, b, None)
    lat.set_param("cg_tgauge_recon", 12)
    x12, _, act12 = window(lq, lat, D, b, n)
    s12, it12, _ = window(lq, lat, D, b, None)
    assert (act8, act12) == (8, 12)
    want = oracle_pair(orc, L, bc, n)
    got = relmax(x8, x12)
    print("L", L, "bc", bc, "window", n, "gate %.2e" % dev, "oracle 12 vs 8 %.3e" % want, "device 12 vs 8 %.3e" % got, "solve iterations", it8, it12)
    assert 0.0 < got <= 10.0 * want, (got, want)
    assert abs(it8 - it12) <= 1      # (two operators 1e-15 apart may cross eps on neighbouring iterations)
    # the solve to eps 1e-16 against the oracle's solution: the 1e-12 and the +-1 iteration tests/test_gpu_cg_rring.py holds its forms to, and the true residual below eps
    xo, ito, rro, st = orc.cg_DdagD(orc.WILSON, Uh, bh, L, KAPPA, 1.0, bc, eps=1e-16)
    err = relmax(s8, xo)
    res = bh - orc.wilson_D(Uh, orc.wilson_D(Uh, s8, L, KAPPA, 1.0, bc), L, KAPPA, 1.0, bc, dagger=True)
    rr = float(np.vdot(res, res).real)
    print("   solve: iterations", it8, "oracle", ito, "rel max diff to the oracle's x %.3e" % err, "true residual %.3e" % rr)
    assert st == 0 and abs(it8 - ito) <= 1
    assert err <= 1e-12, err
    assert rr < 1e-16, rr
    assert np.array_equal(b.download(), bh)


@pytest.mark.parametrize("L", [SMALL, MID, WIDE])
def test_same_bits_with_every_switch_and_across_two_runs(lq, orc, L):
    Uh, bh = problem(orc, L)
    lat, U, D, b = make(lq, L, ANTI, Uh, bh, recon=8)
    n = 3 * lat.get_param("cg_rring") * MULT + 5
    ref, _, act = window(lq, lat, D, b, n)
    sol, its, _ = window(lq, lat, D, b, None)
    assert act == 8
    again, _, _ = window(lq, lat, D, b, n)
    assert np.array_equal(again, ref)
    on = {a: lat.get_param(a) for a in ("xshare_active", "yshare_active", "cg_sweep_alt_active")}      # (what the last launches of the reference run took)
    for key, active, other in (("dslash_xshare", "xshare_active", 0), ("dslash_yshare", "yshare_active", 0), ("cg_sweep_alt", "cg_sweep_alt_active", 0),
                               ("cg_store_keep_mb", None, -1), ("cg_store_keep_mb", None, 0)):
        was = lat.get_param(key)
        live = active is not None and (L[0] == 32 or key == "cg_sweep_alt")      # the shares need 16 lanes per x-row: on 16-wide lattices their keys switch nothing
        if live:
            assert on[active] == 1, key       # on in the reference run: turning it off changes the launches
        lat.set_param(key, other)
        got, _, act = window(lq, lat, D, b, n)
        s2, it2, _ = window(lq, lat, D, b, None)
        if live:
            assert lat.get_param(active) == 0, key
        lat.set_param(key, was)
        assert act == 8
        assert np.array_equal(got, ref) and np.array_equal(s2, sol) and it2 == its, key


def test_a_gate_that_fails_runs_the_12_real_solve(lq, orc):
    L = SMALL
    Uh, bh = problem(orc, L)
    lat, U, D, b = make(lq, L, ANTI, Uh, bh, recon=8)
    n = 3 * lat.get_param("cg_rring") * MULT + 5
    x8, _, act = window(lq, lat, D, b, n)
    assert act == 8
    lat.set_param("tgauge8_gate_e", 17)
    xg, _, actg = window(lq, lat, D, b, n)
    lat.set_param("tgauge8_gate_e", 14)
    lat.set_param("cg_tgauge_recon", 12)
    x12, _, act12 = window(lq, lat, D, b, n)
    assert (actg, act12) == (12, 12)
    assert np.array_equal(xg, x12) and not np.array_equal(x8, x12)
    with pytest.raises(lq.LQCDError):
        lat.set_param("cg_tgauge_recon", 10)
    # unset, the key leaves a lattice of 64 stencil workgroups on 12 reals
    lat2 = lq.Lattice(L)
    for k, v in (("cg_persist", 0), ("cg_small", 0), ("cg_tgauge", 2)):
        lat2.set_param(k, v)
    U2 = lq.Gaugefields(lat2).upload(Uh)
    D2 = lq.Dirac_operator(U2, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": ANTI})
    b2 = lq.Fermionfields(lat2, lq.WILSON).upload(bh)
    assert lat2.get_param("cg_tgauge_recon") == 8
    assert window(lq, lat2, D2, b2, 3)[2] == 12


def test_a_cold_start_runs_in_8_reals(lq, orc):
    L = SMALL
    _, bh = problem(orc, L)
    Uh = orc.unit_gauge(L)
    lat, U, D, b = make(lq, L, ANTI, Uh, bh, recon=8)
    assert lq.tgauge8_deviation(U) <= 1e-14
    x8, it8, act = window(lq, lat, D, b, None)
    assert act == 8
    # the solver's contract: the true residual below eps, the oracle's iteration count to +-1; and the 12-real solve of the same library to the 1e-12 the project holds
    # its CG forms to (unit links decode exactly; the free operator at this kappa is worse conditioned than the hot start, so no bound on x itself is carried over)
    xo, ito, rro, st = orc.cg_DdagD(orc.WILSON, Uh, bh, L, KAPPA, 1.0, ANTI, eps=1e-16)
    res = bh - orc.wilson_D(Uh, orc.wilson_D(Uh, x8, L, KAPPA, 1.0, ANTI), L, KAPPA, 1.0, ANTI, dagger=True)
    assert st == 0 and abs(it8 - ito) <= 1
    assert float(np.vdot(res, res).real) < 1e-16
    lat.set_param("cg_tgauge_recon", 12)
    x12, it12, act12 = window(lq, lat, D, b, None)
    assert act12 == 12 and abs(it12 - it8) <= 1 and relmax(x8, x12) <= 1e-12
