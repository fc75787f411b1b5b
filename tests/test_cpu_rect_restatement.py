"""The numpy restatement of the plaquette + rectangle action (tests/rect_numpy.py) against what is known without it: a cold field, gauge invariance, the oracle's
plaquette action and force at beta_rect = 0, the derivative of its own action by finite differences, and an abelian field with a known rectangle."""
import numpy as np
import pytest

import rect_numpy as rn
from conftest import rel_err

L4 = (4, 4, 4, 4)
LW = rn.lw(5.7)
IWASAKI = rn.c1_action(5.7, -0.331)


@pytest.fixture(scope="module")
def hot(orc):
    return orc.hot_gauge(L4, 811)


def test_cold_field(orc):
    for L in ((4, 4, 4, 4), (4, 6, 2, 4)):
        U, V = orc.unit_gauge(L), float(np.prod(L))
        assert rn.rectangle(U, L) == 1.0 and rn.plaquette(U, L) == 1.0
        for bp, br in (LW, IWASAKI, (1.0, 0.0)):
            assert abs(rn.action(U, L, bp, br) - (-6.0 * V * bp - 12.0 * V * br)) < 1e-12 * V * (abs(bp) + abs(br))
        assert np.abs(rn.ta(rn.to_xyzt(rn.force(U, L, *LW)))).max() < 1e-15


def test_coefficients():
    bp, br = LW
    assert abs(bp + 8.0 * br - 5.7) < 1e-15                       # every improved action here keeps beta_plaq + 8 beta_rect = beta
    bp, br = IWASAKI
    assert abs(bp + 8.0 * br - 5.7) < 1e-14 and abs(br + 0.331 * 5.7) < 1e-15


def test_gauge_rotation(orc):
    L = (4, 6, 4, 4)
    U = orc.hot_gauge(L, 812)
    Ug, g = rn.gauge_transform(U, L, 813)
    assert np.abs(g @ rn.dag(g) - np.eye(3)).max() < 1e-14
    assert np.abs(Ug - U).max() > 0.1
    assert abs(rn.rectangle(Ug, L) - rn.rectangle(U, L)) < 1e-12 * abs(rn.rectangle(U, L)) + 1e-15
    S, Sg = rn.action(U, L, *LW), rn.action(Ug, L, *LW)
    assert abs(S - Sg) < 1e-12 * abs(S)
    G, Gg = rn.to_xyzt(rn.force(U, L, *LW)), rn.to_xyzt(rn.force(Ug, L, *LW))
    assert np.abs(Gg - g @ G @ rn.dag(g)).max() < 1e-12 * np.abs(G).max()       # U_mu(n) (staples) is a sum of loops closed at n


def test_plaquette_limit_is_the_oracle(orc, hot):
    assert abs(rn.action(hot, L4, 5.7, 0.0) - orc.gauge_action(hot, L4, 5.7)) < 1e-12 * abs(orc.gauge_action(hot, L4, 5.7))
    assert rel_err(rn.force(hot, L4, 5.7, 0.0), orc.gauge_force(hot, L4, 5.7)) < 1e-13
    assert abs(rn.plaquette(hot, L4) - orc.plaquette(hot, L4)) < 1e-14


@pytest.mark.parametrize("L,coef", [(L4, LW), (L4, IWASAKI), ((4, 4, 2, 2), LW)])
def test_force_is_the_derivative_of_the_action(orc, L, coef):
    """Central difference of S under U_mu(n) -> exp(i eps T) U_mu(n), eps = 1e-4, against -2 Im tr(T G): truncation ~ eps^2, rounding ~ |S| 1e-16 / eps ~ 1e-9,
    bound 1e-6 max(1, |dS/d eps|).  (4,4,2,2): a 2-long side closes on itself and a link enters one loop twice -- the product rule is the staple sum."""
    U = orc.hot_gauge(L, 811)
    G = rn.force(U, L, *coef)
    eps = 1e-4
    for site, mu, T in rn.fd_rotations(L):
        d = (rn.action(rn.rotate_link(U, site, mu, T, eps), L, *coef) - rn.action(rn.rotate_link(U, site, mu, T, -eps), L, *coef)) / (2.0 * eps)
        pred = rn.fd_prediction(G, site, mu, T)
        assert abs(d - pred) < 1e-6 * max(1.0, abs(d)), (site, mu, d, pred)
        assert abs(d) > 1e-3                                         # a hot field: the derivative is not small


def test_only_the_relative_weight_fixes_the_force(orc, hot):
    """linear in (beta_plaq, beta_rect), and the rectangle part is not a multiple of the plaquette part"""
    Gp, Gr = rn.force(hot, L4, 1.0, 0.0), rn.force(hot, L4, 0.0, 1.0)
    assert rel_err(rn.force(hot, L4, *LW), LW[0] * Gp + LW[1] * Gr) < 1e-14
    c = np.vdot(Gp, Gr) / np.vdot(Gp, Gp)
    assert np.abs(Gr - c * Gp).max() > 0.1 * np.abs(Gr).max()


def test_ta_projection_enters_the_momenta(orc, hot):
    X = rn.ta(rn.to_xyzt(rn.force(hot, L4, *LW)))
    # anti-Hermitian exactly; the trace is three diagonal entries of size <= 4, each rounded once when tr / 3 is taken off: a few 2^-52 * 4
    assert np.abs(X + rn.dag(X)).max() == 0.0 and np.abs(np.trace(X, axis1=-2, axis2=-1)).max() < 1e-14
    assert np.abs(X).max() > 0.1


def test_abelian_flux_field_has_its_known_rectangle(orc):
    L = (6, 4, 4, 8)
    U, th, th2 = rn.flux_field(L, 1, 2)
    assert orc.unitarity_dev(U, L) < 1e-15
    assert abs(rn.plaquette(U, L) - (4.0 + (2.0 * np.cos(th) + 1.0) / 3.0 + (2.0 * np.cos(th2) + 1.0) / 3.0) / 6.0) < 1e-14
    assert abs(rn.rectangle(U, L) - rn.flux_rectangle(th, th2)) < 1e-14
    assert abs(rn.flux_rectangle(th, th2) - 1.0) > 1e-2
