"""The residual ring at depths 16 and 32 (cg_fused = 3, cg_rring = K, cg_rring_mult = M, K M slots; cg.hip cg_batch_px<NT, DEPTH>, cg_run's captured burst of
K M iterations).  16.8.8.4 with cg_tgauge = 2 (the temporal-gauge instances, seam slices half the lattice) and 16.16.16.8 (the plain 12-real instance), cg_small = 0
on both (64 and 512 stencil workgroups), (K, M) = (8, 2), (4, 4), (8, 4).

Fixed windows below, at and above batch boundaries against cg_fused = 2 of the same library, to the 1e-12 the project holds across forms, on the smooth-link
kappa = 0.1285 systems of tests/hard_systems.py (late updates still matter there); the hard-system contract of DESIGN.md section 17 on wilson_cg_16 with the
oracle's C_ref; solves that end at k mod depth = depth - 1, 0, 1 (tests/rring_deep.py, oracle side: tests/test_cpu_cg_recurrence_deep.py) with it == k and x to
1e-10 of the oracle; the same bits from two runs, a split session, graph 0 / 1 and an exhausted solve; the tunables."""
import numpy as np
import pytest

import hard_systems as hs
import rring_deep as rd
import solve_endings as se
from test_gpu_hard_solves import cg, count_in_band, hold

pytestmark = pytest.mark.gpu

IDS = lambda v: ".".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


def context(lq, L, K=8, M=None):
    lat = lq.Lattice(L)
    for k, v in (("cg_persist", 0), ("cg_small", 0), ("cg_tgauge", 2 if tuple(L) == rd.SMALL else 0), ("cg_fused", 3), ("cg_rring", K)):
        lat.set_param(k, v)
    if M is not None:
        lat.set_param("cg_rring_mult", M)
    return lat


def smooth(lq, orc, L, K=8, M=None, maxit=6000, eps=None):
    s = rd.smooth(L)
    lat = context(lq, L, K, M)
    U = lq.Gaugefields(lat).upload(hs.gauge(orc, s))
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": s["kappa"], "boundarycondition": s["bc"], "eps_CG": s["eps"] if eps is None else eps, "MaxCGstep": maxit})
    b = lq.Fermionfields(lat, lq.WILSON).upload(hs.rhs(orc, s))
    return s, lat, U, D, b


def form(lat, fused, K=8, M=1):
    lat.set_param("cg_fused", fused)
    lat.set_param("cg_rring", K)
    lat.set_param("cg_rring_mult", M)


def window(lq, D, b, n):
    x = b.similar()
    lq.lib.check(lq.lib.lib().lqcd_solve_cg_DdagD_fixed(D._h, x._h, b._h, int(n)))
    return x.download()


def active(lat):
    return lat.get_param("cg_rring_active"), lat.get_param("cg_rring_depth_active")


# ------------------------------------------------------------------ 1. fixed windows against cg_fused = 2
@pytest.mark.parametrize("L", rd.LATTICES, ids=IDS)
def test_fixed_windows_agree_with_cg_fused_2(lq, orc, L):
    s, lat, U, D, b = smooth(lq, orc, L)
    form(lat, 2)
    ref = {n: window(lq, D, b, n) for n in rd.ALL_WINDOWS}
    assert active(lat) == (0, 0)
    worst = 0.0
    for K, M in rd.KM:
        form(lat, 3, K, M)
        for n in rd.windows(K * M):
            got = window(lq, D, b, n)
            assert active(lat) == (K, K * M) and lat.get_param("tgauge_active") == (1 if tuple(L) == rd.SMALL else 0)
            err = rd.relmax(got, ref[n])
            worst = max(worst, err)
            print("L", L, "K", K, "M", M, "n", n, "rel max diff %.3e" % err)
            assert err <= 1e-12, (L, K, M, n, err)
    assert np.array_equal(b.download(), hs.rhs(orc, s))
    print("L", L, "largest rel max diff to cg_fused = 2: %.3e" % worst)


# ------------------------------------------------------------------ 2. the hard-system contract
@pytest.mark.parametrize("KM", rd.KM, ids=IDS)
def test_the_hard_system_contract_holds(lq, orc, KM):
    K, M = KM
    s, lat, U, D, b = smooth(lq, orc, rd.SMALL, K, M)
    xh, it, rr = cg(lq, orc, s, D, b)
    assert active(lat) == (K, K * M) and lat.get_param("tgauge_active") == 1
    hold(orc, s, xh, rr, "cg rring K %d M %d" % (K, M))
    count_in_band(s, it, "rring %dx%d" % (K, M))


# ------------------------------------------------------------------ 3. endings
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("r", rd.ending_rows(), ids=lambda r: r["name"])
def test_a_solve_that_ends_next_to_a_batch_boundary(lq, orc, r, graph):
    sc, xo, ito, st = rd.ending(orc, r)
    assert st == 0 and ito == r["k"]
    lat = context(lq, r["L"])
    lat.set_param("graph", graph)
    U = lq.Gaugefields(lat).upload(se.gauge(orc, r["L"]))
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": se.KAPPA, "boundarycondition": se.BC, "eps_CG": sc["eps"], "MaxCGstep": 3000})
    b = lq.Fermionfields(lat, lq.WILSON).upload(se.rhs(orc, r))
    for K, M in rd.KM:
        if r["k"] not in rd.ending_ks(K * M):
            continue
        form(lat, 3, K, M)
        x = b.similar()
        it, rr = lq.solve_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
        err = se.rel_err(x.download(), xo)
        print("%s graph %d K %d M %d: iterations %d (oracle %d), rel err %.3e" % (r["name"], graph, K, M, it, ito, err))
        assert active(lat) == (K, K * M)
        assert it == r["k"], (it, r["k"])
        assert err <= 1e-10, err


# ------------------------------------------------------------------ 4. the same bits where the same launches run
@pytest.mark.parametrize("L", rd.LATTICES, ids=IDS)
def test_two_runs_a_split_session_graph_replay_and_an_exhausted_solve_are_the_same_bits(lq, orc, L):
    s, lat, U, D, b = smooth(lq, orc, L, eps=1e-6 * float(np.vdot(hs.rhs(orc, rd.smooth(L)), hs.rhs(orc, rd.smooth(L))).real))
    for K, M in rd.KM:
        d = K * M
        form(lat, 3, K, M)
        n = d + 5
        w = window(lq, D, b, n)
        assert active(lat) == (K, d)
        assert np.array_equal(window(lq, D, b, n), w)
        xs = b.similar()
        ses = lq.CGSession(D, xs, b)
        for part in (3, d - 1, 3):
            ses.iterate(part)
        ses.close()
        assert np.array_equal(xs.download(), w), (K, M)
        out = []
        for graph in (0, 1):
            lat.set_param("graph", graph)
            x = b.similar()
            it, rr = lq.solve_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
            assert active(lat) == (K, d)      # the depth does not depend on `graph`
            out.append((x.download(), it, [window(lq, D, b, m) for m in (d, d + 1, 2 * d, 3 * d + 5)]))
        lat.set_param("graph", 0)
        print("L", L, "K", K, "M", M, "solve to 1e-6 |b|^2:", out[0][1], "iterations")
        assert out[0][1] == out[1][1] > d and np.array_equal(out[0][0], out[1][0]), (K, M)
        assert all(np.array_equal(a, c) for a, c in zip(out[0][2], out[1][2])), (K, M)
        assert np.array_equal(out[0][2][1], window(lq, D, b, d + 1))
    # an exhausted solve equals the fixed window
    for K, M in rd.KM:
        d = K * M
        for maxit in (d - 1, d, d + 1):
            s2, lat2, U2, D2, b2 = smooth(lq, orc, L, K, M, maxit=maxit, eps=1e-30)
            x = b2.similar()
            with pytest.raises(lq.NotConverged):
                lq.solve_DinvX_(x, lq.DdagD_operator(D2), b2)
            assert active(lat2) == (K, d)
            assert np.array_equal(x.download(), window(lq, D2, b2, maxit)), (K, M, maxit)


# ------------------------------------------------------------------ 5. the tunables
def test_depth_8_is_one_kernel_whatever_K_and_M_and_a_capped_pool_halves_M(lq, orc):
    L = rd.SMALL
    n = 21
    s, lat, U, D, b = smooth(lq, orc, L, 8, 1)
    w8 = window(lq, D, b, n)
    assert active(lat) == (8, 8)
    # a context that never set cg_rring_mult: M = 1 at this volume (<= 1024 stencil workgroups)
    s0, lat0, U0, D0, b0 = smooth(lq, orc, L, 8, None)
    assert np.array_equal(window(lq, D0, b0, n), w8) and active(lat0) == (8, 8)
    # K = 4, M = 2: the ring of 8 under another name -- the same launches
    form(lat0, 3, 4, 2)
    assert np.array_equal(window(lq, D0, b0, n), w8) and active(lat0) == (4, 8)
    # refused values leave the tunable alone
    for bad in (0, 3, 8, -1, 16):
        with pytest.raises(lq.LQCDError):
            lat0.set_param("cg_rring_mult", bad)
        assert lat0.get_param("cg_rring_mult") == 2
    for K in (2, 4, 8):
        for M in (1, 2, 4):
            form(lat0, 3, K, M)
            assert K * M <= 32      # every admissible pair fits the histories
    with pytest.raises(lq.LQCDError):
        lat0.set_param("cg_rring", 16)
    # a pool capped at 4 + 14 fields: K = 8, M = 4 wants 30 more, gets the 14 of M = 2; at 4 + 6: M = 1; at 5: no ring at all
    form(lat, 3, 8, 2)
    w16 = window(lq, D, b, 2 * n)
    for cap, want in ((18, (8, 16)), (10, (8, 8)), (5, (0, 0))):
        sc, latc, Uc, Dc, bc = smooth(lq, orc, L, 8, 4)
        latc.set_param("scratch_max", cap)
        got = window(lq, Dc, bc, 2 * n)
        assert active(latc) == want, (cap, active(latc))
        if want[1] == 16:
            assert np.array_equal(got, w16)
        else:
            assert rd.relmax(got, w16) <= 1e-12
        latc.set_param("scratch_max", 0)
        window(lq, Dc, bc, 2 * n)
        assert active(latc) == (8, 32)
