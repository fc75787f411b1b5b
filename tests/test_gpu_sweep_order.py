"""The reversed sweep of the scalar-addressing Wilson kernel (StencilCall::sweep_rev; stencil.hip dirsplit_s_block) and the CG that alternates it (tunable cg_sweep_alt:
D forwards, D^+ backwards).  A reversed launch gives every workgroup another virtual block of the same map -- same sites, same operations, partials indexed by virtual
block -- so everything here is compared bit for bit with the forward launch of the same library.
Shapes: 16.8.8.4 (one pass, no y split, 64 workgroups, seam slices are half the lattice), 16.16.16.8 with xcd_nsub = 16, xcd_ysplit = 2 (two passes and (y,z) tiles,
512 workgroups: two passes like 32^3 x 64, but split 2 with ty = 1 -- the map 32^3 x 64 resolves to, split 4 with ty = 2, runs on 32.32.8.4 in
tests/test_gpu_fullsize_hints.py), 16.16.16.32 with default settings (2048 workgroups)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KAPPA = 0.141139
ONEPASS = (16, 8, 8, 4)
TWOPASS = (16, 16, 16, 8)
LARGE = (16, 16, 16, 32)
SHAPES = [ONEPASS, TWOPASS, LARGE]
ANTI, PERIODIC = (1, 1, 1, -1), (1, 1, 1, 1)
WINDOWS = (1, 2, 3, 4, 5, 8, 9, 17)
FORMS = ((3, 2), (3, 4), (3, 8), (2, 4))      # (cg_fused, cg_rring)


def make(lq, orc, L, bc, seed=111, eps=1e-16, tg=True):
    lat = lq.Lattice(L)
    if L != LARGE:
        lat.set_param("cg_small", 0)
        lat.set_param("cg_persist", 0)
        lat.set_param("cg_tgauge", 2)
    if L == TWOPASS:
        lat.set_param("xcd_nsub", 16)
        lat.set_param("xcd_ysplit", 2)
    if not tg:
        lat.set_param("cg_tgauge", 0)
    U = lq.Gaugefields(lat).upload(orc.hot_gauge(L, seed))
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": bc, "eps_CG": eps, "MaxCGstep": 3000})
    bh = orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), seed + 1)
    b = lq.Fermionfields(lat, lq.WILSON).upload(bh)
    return lat, U, D, bh, b


def window(lq, D, b, x0h, n):
    """x after n CG iterations from x0 (n = None: the solve to eps) and the iteration count"""
    x = b.similar()
    if x0h is not None:
        x.upload(x0h)
    it = n
    if n is None:
        it, rr = lq.solve_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
    else:
        lq.lib.check(lq.lib.lib().lqcd_solve_cg_DdagD_fixed(D._h, x._h, b._h, int(n)))
    return x.download(), it


def apply_into_nan(lq, lat, D, b, sweep):
    """y = D b into an output pre-filled with NaN; returns (y, <y, y>, sweep_rev_active)"""
    y = b.similar()
    y.upload(np.full(lat.fermion_shape(lq.WILSON), np.nan + 1j * np.nan, dtype=np.complex128))
    lat.set_param("dslash_sweep", sweep)
    lq.mul_(y, D, b)
    act = lat.get_param("sweep_rev_active")
    lat.set_param("dslash_sweep", 0)
    return y.download(), lq.dot(y, y), act


# ------------------------------------------------------------------ 1. the operator
@pytest.mark.parametrize("bc", [ANTI, PERIODIC])
@pytest.mark.parametrize("L", SHAPES)
def test_a_reversed_application_is_the_same_bits(lq, orc, L, bc):
    lat, U, D, bh, b = make(lq, orc, L, bc)
    for op in (D, D.adjoint()):
        fwd, nf, af = apply_into_nan(lq, lat, op, b, 0)
        rev, nr, ar = apply_into_nan(lq, lat, op, b, 1)
        assert (af, ar) == (0, 1)                        # the second launch did walk backwards
        assert not np.isnan(fwd).any() and not np.isnan(rev).any()      # a reversed map that is no permutation leaves NaN behind
        assert np.array_equal(fwd, rev)
        assert nf == nr and nf.real > 0
    assert np.array_equal(b.download(), bh)


# ------------------------------------------------------------------ 2. CG windows
@pytest.mark.parametrize("L", SHAPES)
def test_cg_windows_are_the_same_bits(lq, orc, L):
    lat, U, D, bh, b = make(lq, orc, L, ANTI, seed=201)
    assert lat.get_param("cg_sweep_alt") == 1      # the default
    for fused, K in FORMS:
        lat.set_param("cg_fused", fused)
        lat.set_param("cg_rring", K)
        for n in WINDOWS:
            out = []
            for alt in (0, 1):
                lat.set_param("cg_sweep_alt", alt)
                out.append(window(lq, D, b, None, n)[0])
                assert lat.get_param("tgauge_active") == 1
                assert lat.get_param("cg_rring_active") == (K if fused == 3 else 0)
                assert lat.get_param("cg_sweep_alt_active") == alt
                assert lat.get_param("sweep_rev_active") == alt      # the last stencil launch of a window is a D^+
            assert np.array_equal(out[0], out[1]), (L, fused, K, n)
    assert np.array_equal(b.download(), bh)


@pytest.mark.parametrize("L", SHAPES)
def test_outside_temporal_gauge_every_launch_stays_forward(lq, orc, L):
    # the time-like links of the plain instances carry the streaming hint on their backward use: the CG reverses nothing there
    lat, U, D, bh, b = make(lq, orc, L, ANTI, seed=211, tg=False)
    lat.set_param("cg_sweep_alt", 1)
    for fused, K in FORMS:
        lat.set_param("cg_fused", fused)
        lat.set_param("cg_rring", K)
        window(lq, D, b, None, 5)
        assert lat.get_param("tgauge_active") == 0
        assert lat.get_param("cg_sweep_alt_active") == 0 and lat.get_param("sweep_rev_active") == 0


# ------------------------------------------------------------------ 3. solves
@pytest.mark.parametrize("x0", ["zero", "random"])
@pytest.mark.parametrize("L", SHAPES)
def test_solves_take_the_same_iterations_and_give_the_same_bits(lq, orc, L, x0):
    lat, U, D, bh, b = make(lq, orc, L, ANTI, seed=301, eps=1e-16)
    x0h = None if x0 == "zero" else orc.gaussian_spinor(lat.fermion_shape(lq.WILSON), 777)
    out = []
    for alt in (0, 1):
        lat.set_param("cg_sweep_alt", alt)
        out.append(window(lq, D, b, x0h, None))
        assert lat.get_param("cg_sweep_alt_active") == alt
    assert out[0][1] == out[1][1] and out[0][1] > 10
    assert np.array_equal(out[0][0], out[1][0])


# ------------------------------------------------------------------ 4. graph replay
@pytest.mark.parametrize("L", [TWOPASS, LARGE])
def test_graph_replay_is_the_same_bits(lq, orc, L):
    lat, U, D, bh, b = make(lq, orc, L, ANTI, seed=401)
    out = []
    for graph in (0, 1):
        lat.set_param("graph", graph)
        out.append([window(lq, D, b, None, n)[0] for n in (16, 17)])
        assert lat.get_param("cg_sweep_alt_active") == 1
    lat.set_param("graph", 0)
    assert all(np.array_equal(a, c) for a, c in zip(out[0], out[1]))


# ------------------------------------------------------------------ 5. the form is fixed at set-up
@pytest.mark.parametrize("first", [0, 1])
def test_a_session_keeps_the_order_it_was_set_up_with(lq, orc, first):
    lat, U, D, bh, b = make(lq, orc, TWOPASS, ANTI, seed=601)
    ref = window(lq, D, b, None, 9)[0]
    lat.set_param("cg_sweep_alt", first)
    xs = b.similar()
    ses = lq.CGSession(D, xs, b)
    assert lat.get_param("cg_sweep_alt_active") == first
    ses.iterate(3)
    assert lat.get_param("sweep_rev_active") == first
    lat.set_param("cg_sweep_alt", 1 - first)      # no iteration reads the tunable
    ses.iterate(6)
    assert lat.get_param("sweep_rev_active") == first
    ses.close()
    assert np.array_equal(xs.download(), ref)
