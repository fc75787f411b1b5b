"""The y-share of the scalar-addressing Wilson kernel (tunable dslash_yshare, read-only yshare_active; stencil.hip sdir_wave): with the x-share (XH = 16) and L1 a multiple
of 4 the y wave takes the in-chunk y-neighbours -- rows 0-2 forwards, rows 1-3 backwards -- from the chunk the x wave has loaded, through LDS behind one workgroup barrier, and
loads only row 3's forward and row 0's backward neighbour itself.  Projection and sign stay on the receiving lane, so everything here is compared bit for bit with
dslash_yshare = 0 of the same library, and with the oracle at the bound of the operator tests (1e-13).
Shapes: the smallest at which each edge case exists -- 32.4.8.4 (one chunk per z-plane: both edge rows wrap into the lane's own chunk), 32.8.8.4 (two chunks: one interior
chunk boundary), 32.12.8.4 (three chunks, L1 no power of two), 32.16.16.8 with xcd_nsub = 16, xcd_ysplit = 2 (a two-pass tile map, split 2; 32^3 x 64 itself resolves to split 4, which tests/test_gpu_fullsize_hints.py runs on 32.32.8.4) -- and 16.8.8.4 (XH = 8),
where the gate must decline.  The lane map: tests/test_cpu_yshare_map.py."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

KAPPA = 0.141139
ONE, TWO, THREE, TWOPASS, XH8 = (32, 4, 8, 4), (32, 8, 8, 4), (32, 12, 8, 4), (32, 16, 16, 8), (16, 8, 8, 4)
SHAPES = [ONE, TWO, THREE, TWOPASS]
BCS = [(1, 1, 1, -1), (1, -1, 1, 1), (-1, -1, -1, -1)]
WINDOWS = (1, 2, 3, 8, 9, 17)
FORMS = ((3, 8), (3, 4), (2, 4))      # (cg_fused, cg_rring)
TOL = 1e-13                           # the bound of the operator tests (test_gpu_pipe.py)

_host = {}


def host_fields(orc, lq_shape, L, seed):
    """links and a Gaussian source of a shape: made once and shared; nobody writes them"""
    k = (L, seed)
    if k not in _host:
        _host[k] = (orc.hot_gauge(L, seed), orc.gaussian_spinor(lq_shape, seed + 1))
    return _host[k]


def make(lq, orc, L, bc, seed=111, eps=1e-16, tg=True):
    lat = lq.Lattice(L)
    lat.set_param("cg_small", 0)
    lat.set_param("cg_persist", 0)
    lat.set_param("cg_tgauge", 2 if tg else 0)
    if L == TWOPASS:
        lat.set_param("xcd_nsub", 16)
        lat.set_param("xcd_ysplit", 2)
    Uh, bh = host_fields(orc, lat.fermion_shape(lq.WILSON), L, seed)
    U = lq.Gaugefields(lat).upload(Uh)
    D = lq.Dirac_operator(U, None, {"Dirac_operator": "Wilson", "κ": KAPPA, "boundarycondition": bc, "eps_CG": eps, "MaxCGstep": 3000})
    b = lq.Fermionfields(lat, lq.WILSON).upload(bh)
    return lat, Uh, U, D, bh, b


def apply_into_nan(lq, lat, op, b, yshare):
    """y = op b into an output pre-filled with NaN; returns (y, <y, y>, yshare_active)"""
    y = b.similar()
    y.upload(np.full(lat.fermion_shape(lq.WILSON), np.nan + 1j * np.nan, dtype=np.complex128))
    lat.set_param("dslash_yshare", yshare)
    lq.mul_(y, op, b)
    act = lat.get_param("yshare_active")
    return y.download(), lq.dot(y, y), act


def window(lq, D, b, n):
    """x after n CG iterations from zero (n = None: the solve to eps) and the iteration count"""
    x = b.similar()
    it = n
    if n is None:
        it, rr = lq.solve_DinvX_(x, lq.DdagD_operator(D), b, return_info=True)
    else:
        lq.lib.check(lq.lib.lib().lqcd_solve_cg_DdagD_fixed(D._h, x._h, b._h, int(n)))
    return x.download(), it


# ------------------------------------------------------------------ 1. the operator
@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("L", SHAPES)
def test_operator_is_the_same_bits_and_the_oracle(lq, orc, L, bc):
    lat, Uh, U, D, bh, b = make(lq, orc, L, bc)
    for dag in (False, True):
        op = D.adjoint() if dag else D
        off, noff, aoff = apply_into_nan(lq, lat, op, b, 0)
        on, non, aon = apply_into_nan(lq, lat, op, b, 1)
        assert (aoff, aon) == (0, 1)
        assert lat.get_param("xshare_active") == 1
        assert not np.isnan(off).any() and not np.isnan(on).any()
        assert np.array_equal(off, on)
        assert noff == non and noff.real > 0
        err = rel_err(on, orc.wilson_D(Uh, bh, L, KAPPA, 1.0, bc, dag))
        print("yshare operator", L, bc, dag, "rel err", err)
        assert err < TOL, (L, bc, dag, err)
    assert np.array_equal(b.download(), bh)


# ------------------------------------------------------------------ 2. point sources at the rows that matter
@pytest.mark.parametrize("L", [ONE, TWO])
def test_point_sources_at_the_edge_rows(lq, orc, L):
    bc = (1, -1, 1, 1)                        # antiperiodic in y: the sign is applied by the receiving lane, on the edge rows only
    lat, Uh, U, D, bh, b = make(lq, orc, L, bc)
    shape = lat.fermion_shape(lq.WILSON)      # (spin, t, z, y, x, colour)
    for y in sorted({0, 3, 4 % L[1], L[1] - 1}):      # first / last row of a chunk, the first row of the next chunk (32.4.8.4: y = 4 is y = 0), the last row of the plane
        for x in (0, 1):                      # both parities of the source site
            src = np.zeros(shape, dtype=np.complex128)
            src[:, 1, 2, y, x, :] = (np.arange(12).reshape(4, 3) + 1.0) * (1.0 - 0.5j)
            b.upload(src)
            for dag in (False, True):
                op = D.adjoint() if dag else D
                off, _, aoff = apply_into_nan(lq, lat, op, b, 0)
                on, _, aon = apply_into_nan(lq, lat, op, b, 1)
                assert (aoff, aon) == (0, 1)
                assert not np.isnan(on).any() and np.array_equal(off, on), (x, y, dag)
                err = rel_err(on, orc.wilson_D(Uh, src, L, KAPPA, 1.0, bc, dag))
                assert err < TOL, (x, y, dag, err)


# ------------------------------------------------------------------ 3. the gate
def test_gate_declines_every_row_length_but_16(lq, orc):
    lat, Uh, U, D, bh, b = make(lq, orc, XH8, (-1, -1, 1, -1))
    for op in (D, D.adjoint()):
        off, noff, aoff = apply_into_nan(lq, lat, op, b, 0)
        on, non, aon = apply_into_nan(lq, lat, op, b, 1)
        assert (aoff, aon) == (0, 0)
        assert not np.isnan(on).any() and np.array_equal(off, on) and noff == non
    xs = []
    for yshare in (0, 1):
        lat.set_param("dslash_yshare", yshare)
        xs.append(window(lq, D, b, 9)[0])
        assert lat.get_param("yshare_active") == 0
    assert np.array_equal(xs[0], xs[1])


def test_the_x_share_switched_off_switches_the_y_share_off(lq, orc):
    lat, Uh, U, D, bh, b = make(lq, orc, TWO, (1, -1, 1, -1))
    out = {}
    for xshare in (1, 0):
        lat.set_param("dslash_xshare", xshare)
        for op, name in ((D, "D"), (D.adjoint(), "Ddag")):
            on, non, aon = apply_into_nan(lq, lat, op, b, 1)
            assert lat.get_param("xshare_active") == xshare and aon == xshare      # dslash_yshare = 1 throughout
            assert not np.isnan(on).any()
            out[(xshare, name)] = on
    for name in ("D", "Ddag"):
        assert np.array_equal(out[(1, name)], out[(0, name)])


# ------------------------------------------------------------------ 4. link formats
@pytest.mark.parametrize("fmt", ["s18", "delta"])
def test_other_link_formats_are_the_same_bits(lq, orc, fmt):
    L, bc = TWO, (-1, -1, 1, -1)
    lat, Uh, U, D, bh, b = make(lq, orc, L, bc)
    if fmt == "s18":
        lat.set_param("gauge_recon", 18)
        lat.set_param("dslash_s18", 1)
        Uref, want, takes = Uh, 0, 0       # the 18-real instance would spill with the y-share: it keeps the x-share alone (sdir_yshare_instance)
    else:
        rng = np.random.default_rng(5)
        Uref = Uh + 1e-10 * (rng.standard_normal(Uh.shape) + 1j * rng.standard_normal(Uh.shape)) / 3.0
        U.upload(Uref)
        want, takes = 2, 1                 # 12 + delta keeps three waves per SIMD with the y-share and takes it
    for dag in (False, True):
        op = D.adjoint() if dag else D
        off, noff, aoff = apply_into_nan(lq, lat, op, b, 0)
        on, non, aon = apply_into_nan(lq, lat, op, b, 1)
        assert lat.get_param("recon_active") == want
        assert aoff == 0 and aon == takes and lat.get_param("xshare_active") == 1
        assert not np.isnan(on).any() and np.array_equal(off, on) and noff == non
        assert rel_err(on, orc.wilson_D(Uref, bh, L, KAPPA, 1.0, bc, dag)) < TOL
    xs = []
    for yshare in (0, 1):
        lat.set_param("dslash_yshare", yshare)
        xs.append(window(lq, D, b, 9)[0])
        assert lat.get_param("tgauge_active") == 0 and lat.get_param("yshare_active") == yshare * takes
    assert np.array_equal(xs[0], xs[1])


# ------------------------------------------------------------------ 5. CG windows and solves
@pytest.mark.parametrize("tg", [True, False])
@pytest.mark.parametrize("L", SHAPES)
def test_cg_windows_are_the_same_bits(lq, orc, L, tg):
    lat, Uh, U, D, bh, b = make(lq, orc, L, (1, 1, 1, -1), seed=201, tg=tg)
    for fused, K in FORMS:
        lat.set_param("cg_fused", fused)
        lat.set_param("cg_rring", K)
        for n in WINDOWS:
            out = []
            for v in (0, 1):
                lat.set_param("dslash_yshare", v)
                out.append(window(lq, D, b, n)[0])
                assert lat.get_param("tgauge_active") == (1 if tg else 0)
                assert lat.get_param("cg_rring_active") == (K if fused == 3 else 0)
                assert lat.get_param("xshare_active") == 1 and lat.get_param("yshare_active") == v
            assert not np.isnan(out[1]).any() and np.array_equal(out[0], out[1]), (L, tg, fused, K, n)
    assert np.array_equal(b.download(), bh)


@pytest.mark.parametrize("tg", [True, False])
def test_solves_take_the_same_iterations(lq, orc, tg):
    lat, Uh, U, D, bh, b = make(lq, orc, TWO, (1, 1, 1, -1), seed=301, eps=1e-16, tg=tg)
    out = []
    for yshare in (0, 1):
        lat.set_param("dslash_yshare", yshare)
        out.append(window(lq, D, b, None))
        assert lat.get_param("yshare_active") == yshare
    assert out[0][1] == out[1][1] and out[0][1] > 10
    assert np.array_equal(out[0][0], out[1][0])
