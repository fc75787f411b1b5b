"""Wilson CG in temporal gauge (tunable cg_tgauge; fields.hip gauge_ensure_tgauge, stencil.hip wilson_dirsplit_s_tg, cg.hip cg_setup / cg_finish).
The solve iterates on (U', G b, G x0) with U'_mu(n) = G(n) U_mu(n) G(n + mu)^+ and hands back G^+ x: the same Krylov space in another basis, so every
result is compared with the cg_tgauge = 0 run of the same library -- relative max-norm 1e-12, one order over the 1e-13 operator bound for what accumulates
over a window (the oracle pair of tests/test_tgauge_oracle.py sits at 2e-15).  cg_tgauge = 2 takes the path on small lattices; 16.16.16.32 (2048 stencil
workgroups, beyond cg_small) takes it by default."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

KAPPA = 0.141139
SMALL = (16, 8, 8, 4)          # T = 4: a seam on every fourth slice; 64 stencil workgroups (the cg_small regime)
LARGE = (16, 16, 16, 32)       # 2048 stencil workgroups: the default setting takes the path


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def make(lq, orc, L, bc, seed=111, eps=1e-16):
    lat = lq.Lattice(L)
    lat.set_param("cg_persist", 0)
    Uh = orc.hot_gauge(L, seed)
    U = lq.Gaugefields(lat).upload(Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": bc, "eps_CG": eps, "MaxCGstep": 3000})
    bh = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), seed + 1)
    b = lq.Fermionfields(lat, lq.WILSON).upload(bh)
    return lat, Uh, U, D, bh, b


def window(lq, lat, D, b, x0h, n):
    """x after n CG iterations from x0 (n = None: the solve to eps); returns (x, iterations, tgauge_active)"""
    x = b.similar()
    if x0h is not None:
        x.upload(x0h)
    it = n
    if n is None:
        it, rr = lq.solve_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
    else:
        lq.lib.check(lq.lib.lib().lqcd_solve_cg_DdagD_fixed(D._h, x._h, b._h, int(n)))
    return x.download(), it, lat.get_param("tgauge_active")


@pytest.mark.parametrize("bc", [(1, 1, 1, -1), (1, 1, 1, 1)])
@pytest.mark.parametrize("L", [SMALL, LARGE])
def test_windows_and_solve_equal_the_unrotated_run(lq, orc, L, bc):
    eps = 1e-16
    lat, Uh, U, D, bh, b = make(lq, orc, L, bc, eps=eps)
    on = 2 if L == SMALL else 1          # the large lattice: the default setting
    assert lat.get_param("cg_tgauge") == 1
    x0r = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 777)
    for x0h in (None, x0r):
        for n in (1, 2, 7, 25, None):
            lat.set_param("cg_tgauge", 0)
            ref, it0, act0 = window(lq, lat, D, b, x0h, n)
            lat.set_param("cg_tgauge", on)
            got, it1, act1 = window(lq, lat, D, b, x0h, n)
            err = relmax(got, ref)
            print("L", L, "bc", bc, "x0", "zero" if x0h is None else "random", "n", n, "iters", it0, it1, "active", act0, act1, "rel max diff %.3e" % err)
            assert act0 == 0 and act1 == 1
            assert err <= 1e-12, (L, bc, n, err)
            assert abs(it1 - it0) <= 1, (it0, it1)
            if n is None:
                res = bh - orc.wilson_D(Uh, orc.wilson_D(Uh, got, L, KAPPA, 1.0, bc), L, KAPPA, 1.0, bc, dagger=True)
                rr = float(np.vdot(res, res).real)
                print("   true residual |b - D^+D x|^2 = %.3e (eps %.1e)" % (rr, eps))
                assert rr < eps, rr
    lat.set_param("cg_tgauge", 1)


@pytest.mark.parametrize("L", [SMALL, LARGE])
def test_iteration_forms_agree_on_the_rotated_problem(lq, orc, L):
    """cg_fused 0 / 1 / 2 and cg_defer_x 0 / 1 / 4 (and cg_small 0 / 1) with the path on: every form iterates on the same rotated problem.
    The identities tests/test_gpu_solver_edges.py pins hold bit for bit: for each cg_fused, the cg_defer_x forms (two buffers, ring of four, x every iteration)
    and the cg_small form give np.array_equal solutions and windows.  ACROSS cg_fused the forms never were the same bits -- cg_fused = 0 takes alpha from
    p.q, 1 and 2 from |D p|^2, and 1 updates r from a stored q by another fma sequence than the epilogue of 2; measured with cg_tgauge = 0 on the same
    lattices: 4e-16 apart -- so across them the solutions and windows agree to the 1e-12 of this file, with equal iteration counts."""
    lat, Uh, U, D, bh, b = make(lq, orc, L, (1, 1, 1, -1), seed=961, eps=1e-16)
    res = {}
    for tg in (0, 2):
        lat.set_param("cg_tgauge", tg)
        for fused in (0, 1, 2):
            for defer, small in ((0, 1), (1, 1), (4, 1), (1, 0)):
                lat.set_param("cg_fused", fused)
                lat.set_param("cg_defer_x", defer)
                lat.set_param("cg_small", small)
                sol, it, act = window(lq, lat, D, b, None, None)
                wins = [window(lq, lat, D, b, None, n)[0] for n in (1, 2, 7, 25)]
                assert act == (1 if tg else 0)
                res[(tg, fused, defer, small)] = (sol, it, wins)
    lat.set_param("cg_fused", 2); lat.set_param("cg_defer_x", 1); lat.set_param("cg_small", 1); lat.set_param("cg_tgauge", 1)
    bad = []
    for (tg, fused, defer, small), (sol, it, wins) in res.items():
        own = res[(tg, fused, 1, 1)]
        base = res[(tg, 2, 1, 1)]
        same = np.array_equal(sol, own[0]) and all(np.array_equal(a, c) for a, c in zip(wins, own[2]))
        err = max([relmax(sol, base[0])] + [relmax(a, c) for a, c in zip(wins, base[2])])
        print("cg_tgauge", tg, "cg_fused", fused, "cg_defer_x", defer, "cg_small", small, "iters", it, "same bits as (defer 1, small 1):", same,
              "largest rel max diff to cg_fused = 2: %.3e" % err)
        if tg and not (same and it == base[1] and err <= 1e-12):
            bad.append((fused, defer, small, same, it, err))
    assert not bad, bad


def test_b_is_untouched_and_a_session_equals_the_window(lq, orc):
    lat, Uh, U, D, bh, b = make(lq, orc, LARGE, (1, 1, 1, -1), seed=301)
    x = b.similar()
    lq.solve_DinvX_(x, lq.DdagD_operator(D), b)
    assert lat.get_param("tgauge_active") == 1
    assert np.array_equal(b.download(), bh)
    for n in (7, 8):
        xs = b.similar()
        ses = lq.CGSession(D, xs, b)
        ses.iterate(3)
        ses.iterate(n - 3)
        ses.close()
        assert lat.get_param("tgauge_active") == 1
        assert np.array_equal(b.download(), bh)
        xw, _, _ = window(lq, lat, D, b, None, n)
        assert np.array_equal(xs.download(), xw), n


def test_a_link_update_under_an_open_session_is_refused(lq, orc):
    lat, Uh, U, D, bh, b = make(lq, orc, LARGE, (1, 1, 1, -1), seed=311)
    xs = b.similar()
    ses = lq.CGSession(D, xs, b)
    ses.iterate(2)
    U.upload(orc.hot_gauge(LARGE, 312))
    with pytest.raises(lq.LQCDError):
        ses.iterate(1)
    ses.close()


def test_gate_and_exclusions_leave_the_solve_as_it_was(lq, orc):
    """tgauge_active = 0 and bit-identical results with cg_tgauge = 2 for links off the group, Wilson-clover, r != 1 and a lattice whose geometry the
    scalar-addressing kernel does not take; after a link update between two solves the second one runs on the new field."""
    L, bc = SMALL, (1, 1, 1, -1)
    lat, Uh, U, D, bh, b = make(lq, orc, L, bc, seed=401)

    def both(Dop):
        out = []
        for mode in (0, 2):
            lat.set_param("cg_tgauge", mode)
            out.append(window(lq, lat, Dop, b, None, 9))
        lat.set_param("cg_tgauge", 1)
        return out

    (x0, _, a0), (x2, _, a2) = both(D)
    assert a0 == 0 and a2 == 1 and relmax(x2, x0) <= 1e-12          # the path is on for this lattice ...
    # ... and off for links that are not on the group to 1e-14 (the gate of the 12-real copy, then of the rotated one)
    rng = np.random.default_rng(5)
    Up = Uh + 1e-10 * (rng.standard_normal(Uh.shape) + 1j * rng.standard_normal(Uh.shape)) / 3.0
    U.upload(Up)
    (x0, _, a0), (x2, _, a2) = both(D)
    assert a0 == 0 and a2 == 0 and np.array_equal(x0, x2)
    # a link update between two solves: the second solve uses the new field
    Un = orc.hot_gauge(L, 402)
    U.upload(Un)
    (x0, _, a0), (x2, _, a2) = both(D)
    assert a0 == 0 and a2 == 1 and relmax(x2, x0) <= 1e-12
    xo = orc.cg_DdagD_fixed(orc.WILSON, Un, bh, L, KAPPA, 1.0, bc, niter=9)
    assert relmax(x2, xo) < 1e-9
    # r != 1
    Dr = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "r": 0.7, "boundarycondition": bc, "eps_CG": 1e-16})
    (x0, _, a0), (x2, _, a2) = both(Dr)
    assert a0 == 0 and a2 == 0 and np.array_equal(x0, x2)
    # Wilson-clover
    Dc = lq.Dirac_operator(U, None, {"Dirac_operator": "WilsonClover", "κ": KAPPA, "Clover_coefficient": 1.2, "boundarycondition": bc, "eps_CG": 1e-16})
    (x0, _, a0), (x2, _, a2) = both(Dc)
    assert a0 == 0 and a2 == 0 and np.array_equal(x0, x2)
    # 8^4: a z-plane is half a chunk, the scalar-addressing kernel does not apply
    lat8, Uh8, U8, D8, bh8, b8 = make(lq, orc, (8, 8, 8, 8), bc, seed=403)
    outs = []
    for mode in (0, 2):
        lat8.set_param("cg_tgauge", mode)
        outs.append(window(lq, lat8, D8, b8, None, 9))
    assert outs[1][2] == 0 and np.array_equal(outs[0][0], outs[1][0])


def test_self_partitioned_context_keeps_the_unrotated_solve(lq, orc):
    code = textwrap.dedent("""
        import os, sys, numpy as np
        sys.path.insert(0, os.getcwd())
        import latticeqcd_jl_amd as lq
        from oracle import oracle as orc
        L, K, BC = (16, 8, 8, 4), 0.141139, (1, 1, 1, -1)
        lat = lq.Lattice(L)
        lat.comm_init(lq.comm_unique_id())
        Ud = lq.Gaugefields(lat).upload(orc.hot_gauge(L, 111))
        D = lq.Dirac_operator(Ud, None, {"Dirac_operator": "Wilson", "κ": K, "boundarycondition": BC, "eps_CG": 1e-16})
        b = lq.Fermionfields(lat, lq.WILSON).upload(orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 112))
        out = []
        for mode in (0, 2):
            lat.set_param("cg_tgauge", mode)
            x = b.similar()
            lq.lib.check(lq.lib.lib().lqcd_solve_cg_DdagD_fixed(D._h, x._h, b._h, 9))
            out.append((x.download(), lat.get_param("tgauge_active")))
        assert out[0][1] == 0 and out[1][1] == 0 and np.array_equal(out[0][0], out[1][0])
        print("TGAUGE_SELF_OK")
    """)
    env = dict(os.environ, LQCD_FORCE_PARTITION="8", HSA_ENABLE_IPC_MODE_LEGACY="0", LQCD_HALO_STREAM_MODE="3")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "TGAUGE_SELF_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
