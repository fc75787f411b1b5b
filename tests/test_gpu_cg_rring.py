"""The residual-ring form of the fp64 Wilson CG (cg_fused = 3, tunable cg_rring = K; cg.hip cg_enqueue_rring / cg_batch_px, stencil.hip sdir_wave's separate
update source and recurrence mode).  D p is formed by s' = D r' + beta s from the residual D^+ has just written, p and x are brought up to date once per K iterations.
Compared with cg_fused = 2 of the same library to the 1e-12 the project holds across cg_fused forms (tests/test_gpu_tgauge.py), iteration counts within +-1;
bit for bit wherever the same launches run.  16.8.8.4 (cg_small = 0, cg_tgauge = 2: seam slices are half the lattice, 64 workgroups) and 16.16.16.32 (default
settings: 2048 workgroups, the temporal-gauge path as the flagship lattice takes it).
The same forms on an ill-conditioned system (1073 iterations, accuracy held against the oracle): tests/test_gpu_hard_solves.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KAPPA = 0.141139
SMALL = (16, 8, 8, 4)
LARGE = (16, 16, 16, 32)
WINDOWS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 25)
ANTI, PERIODIC = (1, 1, 1, -1), (1, 1, 1, 1)


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def make(lq, orc, L, bc, seed=111, eps=1e-16, maxit=3000, tg=True):
    lat = lq.Lattice(L)
    lat.set_param("cg_persist", 0)
    if L != LARGE:
        lat.set_param("cg_small", 0)
    lat.set_param("cg_tgauge", (2 if L != LARGE else 1) if tg else 0)
    Uh = orc.hot_gauge(L, seed)
    U = lq.Gaugefields(lat).upload(Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": bc, "eps_CG": eps, "MaxCGstep": maxit})
    bh = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), seed + 1)
    b = lq.Fermionfields(lat, lq.WILSON).upload(bh)
    return lat, Uh, U, D, bh, b


def form(lat, fused, K=4):
    lat.set_param("cg_fused", fused)
    lat.set_param("cg_rring", K)


def window(lq, lat, D, b, x0h, n):
    """x after n CG iterations from x0 (n = None: the solve to eps); returns (x, iterations, cg_rring_active)"""
    x = b.similar()
    if x0h is not None:
        x.upload(x0h)
    it = n
    if n is None:
        it, rr = lq.solve_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
    else:
        lq.lib.check(lq.lib.lib().lqcd_solve_cg_DdagD_fixed(D._h, x._h, b._h, int(n)))
    return x.download(), it, lat.get_param("cg_rring_active")


# ------------------------------------------------------------------ 1. forms agree, 2. true residual
@pytest.mark.parametrize("x0", ["zero", "random"])
@pytest.mark.parametrize("tg", [0, 1])
@pytest.mark.parametrize("bc", [ANTI, PERIODIC])
@pytest.mark.parametrize("L", [SMALL, LARGE])
def test_forms_agree_and_the_true_residual_is_below_eps(lq, orc, L, bc, tg, x0):
    eps = 1e-16
    lat, Uh, U, D, bh, b = make(lq, orc, L, bc, eps=eps, tg=bool(tg))
    assert lat.get_param("cg_fused") == 3 and lat.get_param("cg_rring") in (2, 4, 8)      # the defaults
    x0h = None if x0 == "zero" else orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 777)
    runs = (None,) + WINDOWS
    form(lat, 2)
    ref = {n: window(lq, lat, D, b, x0h, n) for n in runs}
    assert all(r[2] == 0 for r in ref.values())
    assert lat.get_param("tgauge_active") == tg
    worst = 0.0
    for K in (2, 4, 8):
        form(lat, 3, K)
        for n in runs:
            got, it, act = window(lq, lat, D, b, x0h, n)
            err = relmax(got, ref[n][0])
            worst = max(worst, err)
            print("L", L, "bc", bc, "tgauge", tg, "x0", x0, "K", K, "n", n, "iters", ref[n][1], it, "rel max diff %.3e" % err)
            assert act == K and lat.get_param("tgauge_active") == tg
            assert err <= 1e-12, (L, bc, tg, x0, K, n, err)
            assert abs(it - ref[n][1]) <= 1, (it, ref[n][1])
            if n is None:
                res = bh - orc.wilson_D(Uh, orc.wilson_D(Uh, got, L, KAPPA, 1.0, bc), L, KAPPA, 1.0, bc, dagger=True)
                rr = float(np.vdot(res, res).real)
                print("   true residual |b - D^+D x|^2 = %.3e (eps %.1e)" % (rr, eps))
                assert rr < eps, rr
    assert np.array_equal(b.download(), bh)
    print("largest rel max diff to cg_fused = 2: %.3e" % worst)


# ------------------------------------------------------------------ 3. same bits where the same launches run
@pytest.mark.parametrize("L", [SMALL, LARGE])
def test_two_runs_a_split_session_and_a_window_behind_a_solve_are_the_same_bits(lq, orc, L):
    lat, Uh, U, D, bh, b = make(lq, orc, L, ANTI, seed=301)
    for K in (2, 4, 8):
        form(lat, 3, K)
        w9, _, act = window(lq, lat, D, b, None, 9)
        assert act == K
        assert np.array_equal(window(lq, lat, D, b, None, 9)[0], w9)
        xs = b.similar()
        ses = lq.CGSession(D, xs, b)
        for n in (3, 5, 1):
            ses.iterate(n)
        ses.close()
        assert np.array_equal(xs.download(), w9), K
        s1, it1, _ = window(lq, lat, D, b, None, None)
        assert np.array_equal(window(lq, lat, D, b, None, 9)[0], w9), K      # a window after a converged solve on the same context
        s2, it2, _ = window(lq, lat, D, b, None, None)
        assert it1 == it2 and np.array_equal(s1, s2)
    assert np.array_equal(b.download(), bh)


@pytest.mark.parametrize("maxit", [5, 6, 7])
def test_an_exhausted_solve_equals_the_fixed_window(lq, orc, maxit):
    lat, Uh, U, D, bh, b = make(lq, orc, LARGE, ANTI, seed=311, eps=1e-30, maxit=maxit)
    for K in (2, 4, 8):
        form(lat, 3, K)
        x = b.similar()
        with pytest.raises(lq.NotConverged):
            lq.solve_DinvX_(x, lq.DdagD_operator(D), b)
        assert lat.get_param("cg_rring_active") == K
        assert np.array_equal(x.download(), window(lq, lat, D, b, None, maxit)[0]), (K, maxit)


def test_graph_replay_is_the_same_bits(lq, orc):
    L = (16, 16, 16, 16)
    lat, Uh, U, D, bh, b = make(lq, orc, L, ANTI, seed=321)
    for K in (2, 4, 8):
        form(lat, 3, K)
        out = []
        for graph in (0, 1):
            lat.set_param("graph", graph)
            sol, it, act = window(lq, lat, D, b, None, None)
            assert act == K      # K does not depend on `graph`
            out.append((sol, it, [window(lq, lat, D, b, None, n)[0] for n in (8, 9, 16, 25)]))
        lat.set_param("graph", 0)
        assert out[0][1] == out[1][1] and np.array_equal(out[0][0], out[1][0]), K
        assert all(np.array_equal(a, c) for a, c in zip(out[0][2], out[1][2])), K


# ------------------------------------------------------------------ 4. the stencil epilogue
def epilogue(lq, D, dst, src, inp, dagger, mode, tgauge, coef, done=0):
    n2 = C.c_double(0)
    lq.lib.check(lq.lib.lib().lqcd_bench_stencil_epilogue(D._h, dst._h, src._h if src is not None else None, inp._h, int(dagger), int(mode), int(tgauge),
                                                          C.c_double(coef), int(done), C.byref(n2)))
    return n2.value


@pytest.mark.parametrize("tgauge", [0, 1])
@pytest.mark.parametrize("bc", [ANTI, PERIODIC])
def test_epilogue_separate_source_recurrence_and_done_flag(lq, orc, bc, tgauge):
    L = SMALL
    lat, Uh, U, D, bh, b = make(lq, orc, L, bc, seed=401)
    shape = lat.fermion_shape(lq.WILSON)
    vh, rh, sh = (orc.gaussian_spinor(shape, s) for s in (402, 403, 404))
    new = lambda h: lq.Fermionfields(lat, lq.WILSON).upload(h)
    v = new(vh)
    alpha, beta = 0.37, 0.81
    # update-mode D^+: source != destination gives the bits of the in-place launch, and leaves the source alone
    r_in = new(rh)
    n_in = epilogue(lq, D, r_in, r_in, v, 1, 1, tgauge, alpha)
    r_src, r_dst = new(rh), new(sh)
    n_sep = epilogue(lq, D, r_dst, r_src, v, 1, 1, tgauge, alpha)
    assert np.array_equal(r_dst.download(), r_in.download())
    assert np.array_equal(r_src.download(), rh)
    assert n_sep == n_in
    assert not np.array_equal(r_in.download(), rh)
    # recurrence-mode D = D r from a plain launch + beta s on the host; |s|^2 from its partials
    r = new(rh)
    plain = new(sh)
    epilogue(lq, D, plain, None, r, 0, 0, tgauge, 0.0)
    want = plain.download() + beta * sh
    s = new(sh)
    n_rec = epilogue(lq, D, s, None, r, 0, 2, tgauge, beta)
    got = s.download()
    err = relmax(got, want)
    nerr = abs(n_rec - float(np.vdot(got, got).real)) / float(np.vdot(got, got).real)
    print("bc", bc, "tgauge entry", tgauge, "recurrence mode: rel max diff %.3e, |s|^2 rel diff %.3e" % (err, nerr))
    assert err <= 1e-13 and nerr <= 1e-13
    if not tgauge:      # (the plain entry computes the caller's operator)
        assert relmax(plain.download(), orc.wilson_D(Uh, rh, L, KAPPA, 1.0, bc)) <= 1e-13
    # the done flag: the launch leaves s untouched
    s2 = new(sh)
    epilogue(lq, D, s2, None, r, 0, 2, tgauge, beta, done=1)
    assert np.array_equal(s2.download(), sh)


# ------------------------------------------------------------------ 5. fallbacks
def test_everything_else_runs_as_cg_fused_2(lq, orc):
    L, bc = LARGE, ANTI
    lat, Uh, U, D, bh, b = make(lq, orc, L, bc, seed=501)
    with pytest.raises(lq.LQCDError):
        lat.set_param("cg_rring", 3)
    assert lat.get_param("cg_rring") in (2, 4, 8)

    def both(latx, run):
        out = []
        for fused in (2, 3):
            latx.set_param("cg_fused", fused)
            out.append(run())
            assert latx.get_param("cg_rring_active") == 0
        assert np.array_equal(out[0], out[1])

    assert window(lq, lat, D, b, None, 9)[2] > 0           # the form is on for this lattice ...
    lat.set_param("cg_rring", 0)                            # ... off by its tunable
    both(lat, lambda: window(lq, lat, D, b, None, 9)[0])
    lat.set_param("cg_rring", 4)
    Dr = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "r": 0.7, "boundarycondition": bc, "eps_CG": 1e-16})
    both(lat, lambda: window(lq, lat, Dr, b, None, 9)[0])
    Dc = lq.Dirac_operator(U, None, {"Dirac_operator": "WilsonClover", "κ": KAPPA, "Clover_coefficient": 1.2, "boundarycondition": bc, "eps_CG": 1e-16})
    both(lat, lambda: window(lq, lat, Dc, b, None, 9)[0])
    Ds = lq.Dirac_operator(U, None, {"Dirac_operator": "Staggered", "mass": 0.1, "boundarycondition": bc, "eps_CG": 1e-16})
    bs = lq.Fermionfields(lat, lq.STAGGERED).upload(orc.gaussian_spinor(lat.fermion_shape(lq.STAGGERED), 502))
    both(lat, lambda: window(lq, lat, Ds, bs, None, 9)[0])
    # the cg_small regime (64 stencil workgroups, cg_small left at its default)
    lats = lq.Lattice(SMALL)
    Us = lq.Gaugefields(lats).upload(orc.hot_gauge(SMALL, 503))
    Dsm = lq.Dirac_operator(Us, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": bc, "eps_CG": 1e-16})
    bsm = lq.Fermionfields(lats, lq.WILSON).upload(orc.gaussian_spinor(lats.fermion_shape(lq.WILSON), 504))
    both(lats, lambda: window(lq, lats, Dsm, bsm, None, 9)[0])
    # 8^4: a z-plane is half a chunk, the scalar-addressing kernel does not apply
    lat8, Uh8, U8, D8, bh8, b8 = make(lq, orc, (8, 8, 8, 8), bc, seed=505)
    both(lat8, lambda: window(lq, lat8, D8, b8, None, 9)[0])


def test_an_in_process_grid_runs_as_cg_fused_2(lq, orc):
    gL, pe, bc = (8, 8, 8, 16), (1, 1, 1, 2), ANTI
    Uh = orc.hot_gauge(gL, 511)
    bh = orc.gaussian_spinor(orc.wilson_shape(gL), 512)
    lats = [lq.Lattice(gL, pe, r) for r in range(2)]
    lq.link_local(lats)
    Us = [lq.Gaugefields(lat).upload(lq.pegrid.local_view(Uh, lat.local_L, lat.origin, lead=1)) for lat in lats]
    Ds = [lq.Dirac_operator(Ud, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": bc}) for Ud in Us]
    bs = [lq.Fermionfields(lat, lq.WILSON).upload(lq.pegrid.local_view(bh, lat.local_L, lat.origin, lead=1)) for lat in lats]
    out = []
    for fused in (2, 3):
        for lat in lats:
            lat.set_param("cg_fused", fused)
        xs = [b.similar() for b in bs]
        it, rr = lq.mdom_solve_cg(Ds, xs, bs, eps=1e-16)
        out.append((it, [x.download() for x in xs]))
        assert all(lat.get_param("cg_rring_active") == 0 for lat in lats)
    assert out[0][0] == out[1][0] and all(np.array_equal(a, c) for a, c in zip(out[0][1], out[1][1]))
    with pytest.raises(lq.LQCDError):
        lats[0].set_param("cg_rring", 3)
